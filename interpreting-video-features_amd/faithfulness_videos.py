"""Deletion and insertion curves (Petsiuk et al. 2018), the faithfulness measure that compares the attribution
methods: an EXTENSION without a counterpart in the reference, in the shape of `shapley_videos.ShapleyVideo`.

`FaithfulnessVideo(model)(clip, attribution, index)` returns `(result, output [1,K])`, `result` a dict of numpy arrays
for the one clip: `ranks` [P], `deletion`, `insertion` [J+1] (the class score along each curve), `del_auc`, `ins_auc`,
`del_auc_norm`, `ins_auc_norm` and `score_x`.  The cells of `grid` = (gt, gh, gw) -- by default (T, 1, 1), the frames --
are ranked by the attribution (a higher value = more important; a frame profile [T], cells [gt,gh,gw] or [T,gh,gw], or
a pixel map [T,H,W], which is pooled to the cells), then frozen per pixel in that order (deletion), or released in that
order from the fully frozen clip (insertion), `step` cells per forward pass; a cell is expanded to pixels with the
bilinear + Gaussian map of the spacetime search (`sigma` input pixels).  The AUC is the trapezoid over the fraction of
cells; the normalised one puts the fully frozen clip at 0 and the clip at 1.  A faithful attribution has a low deletion
and a high insertion AUC.  Everything runs through the HIP plan (csrc/curve_ops.hip ranks the cells, stages the
perturbed clips and reduces the scores); there is no backward pass and nothing falls back to PyTorch.
"""
import numpy as np
import torch

import ivf_lib as L
from grad_cam_videos import _arch, _unwrap


class FaithfulnessVideo:
    def __init__(self, model, grid=None, sigma=None, step=1, order="morf", class_dict=None, use_cuda=True,
                 archType="I3D"):
        self.model = _unwrap(model)
        self.archType = archType
        self.cuda = use_cuda
        self.class_dict = class_dict
        self.grid, self.sigma, self.step, self.order = grid, sigma, int(step), order
        self.last = None                # the engine's whole result dict of the last call (device tensors)
        if self.cuda:
            self.model = self.model.cuda()

    def __call__(self, input, attribution, index=None):
        _arch(self.archType)
        x = input.cuda() if self.cuda else input
        L.require_gpu(x)
        if x.shape[0] != 1:
            raise L.IvfError("FaithfulnessVideo takes one clip [1,C,T,H,W], as GradCamVideo does")
        attr = torch.as_tensor(np.asarray(attribution) if not torch.is_tensor(attribution) else attribution)
        attr = attr.to(x.device, torch.float32)
        if attr.dim() in (1, 3):        # one clip's attribution without the batch axis
            attr = attr[None]
        eng = self.model._engine_for(x, min_batch=32)                   # the rows of one clip fill the plan
        output = eng.forward(x)
        target = [int(index)] if index is not None else eng.argmax(output)
        self.last = eng.faithfulness(x, target, attr, grid=self.grid, sigma=self.sigma, step=self.step, order=self.order)
        r = {k: v[0].cpu().numpy() for k, v in self.last.items()}
        return dict(ranks=r["curve_ranks"].astype(np.int64) & 0xFFFF, deletion=r["del_scores"], insertion=r["ins_scores"],
                    del_auc=r["del_auc"], ins_auc=r["ins_auc"], del_auc_norm=r["del_auc_norm"],
                    ins_auc_norm=r["ins_auc_norm"], score_x=r["score_x"]), output
