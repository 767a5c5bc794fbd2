"""Shapley value sampling for video (Castro et al. 2009; Strumbelj & Kononenko 2014), an EXTENSION without a
counterpart in the reference, in the shape of `rise_videos.RiseVideo`.

`ShapleyVideo(model)(clip, index)` returns `(shap_map float32 [T,H,W], output [1,K])`: the players are the cells of
`grid` = (gt, gh, gw) -- by default (T, 1, 1), the frames -- and a coalition is the set of frozen cells, expanded to
pixels with the bilinear + Gaussian map of the spacetime search (`sigma` input pixels) and applied as the per-pixel
freeze.  Along each of `n_perms` permutations the cells are frozen one after another and every prefix is scored by a
forward pass only (`n_perms` (cells + 1) of them); a cell's value is the mean drop of the class score on its entry,
positive where freezing the cell lowers the score, and the values of a clip sum to score(clip) - score(fully frozen clip)
(`.last["shap_total"]`).  The permutations come from a counter-based integer hash of (`seed`, permutation, cell), with
`antithetic` every odd one the reverse of the one before: the same `seed` gives the same permutations for every clip, on
every run.  Everything runs through the HIP plan (csrc/shapley_ops.hip ranks the cells, stages the perturbed clips and
reduces the scores); there is no backward pass and nothing falls back to PyTorch.
"""
import numpy as np

import ivf_lib as L
from grad_cam_videos import _arch, _unwrap


class ShapleyVideo:
    def __init__(self, model, class_dict=None, use_cuda=True, n_perms=64, grid=None, sigma=None, seed=0, antithetic=True,
                 archType="I3D"):
        self.model = _unwrap(model)
        self.archType = archType
        self.cuda = use_cuda
        self.class_dict = class_dict
        self.n_perms, self.grid, self.sigma, self.seed = int(n_perms), grid, sigma, int(seed)
        self.antithetic = bool(antithetic)
        self.last = None                # the engine's whole result dict of the last call (device tensors)
        if self.cuda:
            self.model = self.model.cuda()

    def __call__(self, input, index=None):
        _arch(self.archType)
        x = input.cuda() if self.cuda else input
        L.require_gpu(x)
        if x.shape[0] != 1:
            raise L.IvfError("ShapleyVideo takes one clip [1,C,T,H,W], as GradCamVideo does")
        eng = self.model._engine_for(x, min_batch=32)                   # the rows of one clip fill the plan
        output = eng.forward(x)
        target = [int(index)] if index is not None else eng.argmax(output)
        self.last = eng.shapley(x, target, n_perms=self.n_perms, grid=self.grid, sigma=self.sigma, seed=self.seed,
                                antithetic=self.antithetic)
        return self.last["shap_map"][0].cpu().numpy().astype(np.float32), output
