"""KernelSHAP (Lundberg & Lee 2017) and LIME (Ribeiro et al. 2016) for video, EXTENSIONS without a counterpart in the
reference, in the shape of `shapley_videos.ShapleyVideo`.

`KernelShapVideo(model)(clip, index)` and `LimeVideo(model)(clip, index)` return `(map float32 [T,H,W], output [1,K])`.
The players are the cells of `grid` = (gt, gh, gw) -- by default (T, 1, 1), the frames -- and a sample row freezes a set
of cells, expanded to pixels with the bilinear + Gaussian map of the spacetime search (`sigma` input pixels) and applied
as the per-pixel freeze.  Every row is scored by a forward pass only; a linear model of the score drop in the frozen
cells is then fitted by least squares in fp64 on the device, and a cell's coefficient is positive where freezing the
cell lowers the score.

KernelSHAP draws the coalition sizes from the Shapley kernel (`paired`: every odd row is the complement of the one
before it) and solves the efficiency constraint exactly: the values of a clip sum to score(clip) - score(fully frozen
clip) (`.last["kshap_total"]`).  LIME draws Bernoulli(`p`) rows -- RISE's masks --, weighs a row by
exp(-D^2 / (2 `width`^2)) of its distance D to the clip and fits a ridge regression (`ridge`) with a free intercept.
`.last["*_ok"]` is 0, and the map NaN, where a score was not finite or the sampled system is singular;
`.last["*_r2"]` is the weighted R^2 of the fit.  The rows come from a counter-based integer hash of (`seed`, row, cell):
the same `seed` gives the same rows for every clip, on every run.  Everything runs through the HIP plan
(csrc/linsur_ops.hip samples the rows, stages the perturbed clips, builds the normal equations and solves them by a
Cholesky factorisation); there is no backward pass and nothing falls back to PyTorch.
"""
import numpy as np

import ivf_lib as L
from grad_cam_videos import _arch, _unwrap


class _SurrogateVideo:
    _name = None        # the engine call and the prefix of its result keys

    def __init__(self, model, class_dict, use_cuda, archType, **kw):
        self.model = _unwrap(model)
        self.archType = archType
        self.cuda = use_cuda
        self.class_dict = class_dict
        self.kw = kw
        self.last = None                # the engine's whole result dict of the last call (device tensors)
        if self.cuda:
            self.model = self.model.cuda()

    def __call__(self, input, index=None):
        _arch(self.archType)
        x = input.cuda() if self.cuda else input
        L.require_gpu(x)
        if x.shape[0] != 1:
            raise L.IvfError(f"{type(self).__name__} takes one clip [1,C,T,H,W], as GradCamVideo does")
        eng = self.model._engine_for(x, min_batch=32)                   # the rows of one clip fill the plan
        output = eng.forward(x)
        target = [int(index)] if index is not None else eng.argmax(output)
        call, prefix = self._name
        self.last = getattr(eng, call)(x, target, **self.kw)
        return self.last[prefix + "_map"][0].cpu().numpy().astype(np.float32), output


class KernelShapVideo(_SurrogateVideo):
    _name = ("kernelshap", "kshap")

    def __init__(self, model, class_dict=None, use_cuda=True, n_samples=256, grid=None, sigma=None, seed=0, paired=True,
                 archType="I3D"):
        super().__init__(model, class_dict, use_cuda, archType, n_samples=int(n_samples), grid=grid, sigma=sigma,
                         seed=int(seed), paired=bool(paired))


class LimeVideo(_SurrogateVideo):
    _name = ("lime", "lime")

    def __init__(self, model, class_dict=None, use_cuda=True, n_samples=1024, p=0.5, grid=None, sigma=None, seed=0,
                 width=0.25, ridge=1.0, archType="I3D"):
        super().__init__(model, class_dict, use_cuda, archType, n_samples=int(n_samples), p=p, grid=grid, sigma=sigma,
                         seed=int(seed), width=width, ridge=ridge)
