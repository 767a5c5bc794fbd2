"""RISE random-mask saliency for video (Petsiuk et al. 2018), an EXTENSION without a counterpart in the reference
(DESIGN 14), in the shape of `integrated_gradients_videos.IntegratedGradientsVideo`.

`RiseVideo(model)(clip, index)` returns `(rise_map float32 [T,H,W], output [1,K])`: the clip is perturbed by `n_masks`
random coarse masks on `grid` = (gt, gh, gw) -- each cell frozen with probability `p`, the grid expanded to pixels with
the bilinear + Gaussian map of the spacetime search (`sigma` input pixels) and applied as the per-pixel freeze -- and
scored by a forward pass only; a cell's importance is the mean drop of the class score over the masks that froze it.
The masks come from a counter-based integer hash of (`seed`, mask, cell): the same `seed` gives the same masks for
every clip, on every run.  Everything runs through the HIP plan (csrc/rise_ops.hip stages the perturbed clips and
reduces the scores); there is no backward pass and nothing falls back to PyTorch.
"""
import numpy as np

import ivf_lib as L
from grad_cam_videos import _arch, _unwrap


class RiseVideo:
    def __init__(self, model, class_dict=None, use_cuda=True, n_masks=1024, p=0.5, grid=None, sigma=None, seed=0,
                 archType="I3D"):
        self.model = _unwrap(model)
        self.archType = archType
        self.cuda = use_cuda
        self.class_dict = class_dict
        self.n_masks, self.p, self.grid, self.sigma, self.seed = int(n_masks), p, grid, sigma, int(seed)
        self.last = None                # the engine's whole result dict of the last call (device tensors)
        if self.cuda:
            self.model = self.model.cuda()

    def __call__(self, input, index=None):
        _arch(self.archType)
        x = input.cuda() if self.cuda else input
        L.require_gpu(x)
        if x.shape[0] != 1:
            raise L.IvfError("RiseVideo takes one clip [1,C,T,H,W], as GradCamVideo does")
        eng = self.model._engine_for(x, min_batch=max(1, min(32, self.n_masks)))    # the masks of one clip fill the plan
        output = eng.forward(x)
        target = [int(index)] if index is not None else eng.argmax(output)
        self.last = eng.rise(x, target, n_masks=self.n_masks, p=self.p, grid=self.grid, sigma=self.sigma, seed=self.seed)
        return self.last["rise_map"][0].cpu().numpy().astype(np.float32), output
