"""Integrated Gradients for video, an EXTENSION without a counterpart in the reference, in the shape of
`grad_cam_videos.GradCamVideo`.

`IntegratedGradientsVideo(model)(clip, index)` returns `(ig_map float32 [T,H,W], output [1,K])`: the attribution of the
class score (post-softmax where the model has a softmax, as Grad-CAM's) to every pixel of every frame, integrated along
the straight path from a baseline clip with `steps` midpoint nodes, and the model's output on the clip.  The map sums
to f(clip) - f(baseline) up to the quadrature error, which `last["ig_gap"]` reports.  Baselines: 'frozen' (every frame =
frame 0, the fully frozen clip init_mask('central') normalises by, mask.py:123-128: frame 0's attribution is exactly
0) and 'constant' (black).  The path points run through the HIP plan's forward and backward (csrc/ig_ops.hip stages
them and accumulates); nothing falls back to autograd.
"""
import numpy as np

import ivf_lib as L
from grad_cam_videos import _arch, _unwrap


class IntegratedGradientsVideo:
    def __init__(self, model, class_dict=None, use_cuda=True, steps=32, baseline="frozen", archType="I3D"):
        self.model = _unwrap(model)
        self.archType = archType
        self.cuda = use_cuda
        self.class_dict = class_dict
        self.steps = int(steps)
        self.baseline = baseline
        self.last = None                # the engine's whole result dict of the last call (device tensors)
        if self.cuda:
            self.model = self.model.cuda()

    def __call__(self, input, index=None):
        _arch(self.archType)
        x = input.cuda() if self.cuda else input
        L.require_gpu(x)
        if x.shape[0] != 1:
            raise L.IvfError("IntegratedGradientsVideo takes one clip [1,C,T,H,W], as GradCamVideo does")
        eng = self.model._engine_for(x)
        output = eng.forward(x)
        target = [int(index)] if index is not None else eng.argmax(output)
        self.last = eng.ig(x, target, steps=self.steps, baseline=self.baseline)
        return self.last["ig_map"][0].cpu().numpy().astype(np.float32), output
