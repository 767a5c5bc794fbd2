"""SmoothGrad, SmoothGrad^2 and VarGrad for video (Smilkov et al. 2017; Hooker et al. 2019), an EXTENSION without a
counterpart in the reference, in the shape of `integrated_gradients_videos.IntegratedGradientsVideo`.

`SmoothGradVideo(model)(clip, index)` returns `(map float32 [T,H,W], output [1,K])`: the gradient of the class score
(post-softmax where the model has a softmax, as Grad-CAM's) with respect to every pixel, taken at `n_samples` noisy
copies clip + sigma z_k, sigma = `level` * (max(clip) - min(clip)), and reduced over the samples and the channels.
`kind` picks the map: 'smoothgrad' = sum_c |mean_k g|, 'sq' = sum_c mean_k g^2, 'var' = sum_c of the unbiased variance
of g over the samples; `.last` keeps all three with their frame sums.  `n_samples=1, level=0` is plain gradient
saliency.  The noise comes from a counter-based integer hash of (`seed`, sample, element): the same `seed` gives the
same noise for every clip, on every run.  Everything runs through the HIP plan's forward and backward
(csrc/smoothgrad_ops.hip stages the noisy clips and accumulates the moments); nothing falls back to autograd.
"""
import numpy as np

import ivf_lib as L
from grad_cam_videos import _arch, _unwrap

KINDS = {"smoothgrad": "sg_map", "sq": "sq_map", "var": "var_map"}


class SmoothGradVideo:
    def __init__(self, model, class_dict=None, use_cuda=True, n_samples=32, level=0.15, seed=0, kind="smoothgrad",
                 archType="I3D"):
        if kind not in KINDS:
            raise L.IvfError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
        self.model = _unwrap(model)
        self.archType = archType
        self.cuda = use_cuda
        self.class_dict = class_dict
        self.n_samples, self.level, self.seed, self.kind = int(n_samples), float(level), int(seed), kind
        self.last = None                # the engine's whole result dict of the last call (device tensors)
        if self.cuda:
            self.model = self.model.cuda()

    def __call__(self, input, index=None):
        _arch(self.archType)
        x = input.cuda() if self.cuda else input
        L.require_gpu(x)
        if x.shape[0] != 1:
            raise L.IvfError("SmoothGradVideo takes one clip [1,C,T,H,W], as GradCamVideo does")
        eng = self.model._engine_for(x, min_batch=max(1, min(32, self.n_samples)))  # the samples of one clip fill the plan
        output = eng.forward(x)
        target = [int(index)] if index is not None else eng.argmax(output)
        self.last = eng.smoothgrad(x, target, n_samples=self.n_samples, level=self.level, seed=self.seed)
        return self.last[KINDS[self.kind]][0].cpu().numpy().astype(np.float32), output
