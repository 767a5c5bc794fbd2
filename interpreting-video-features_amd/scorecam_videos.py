"""Score-CAM for video (Wang et al., CVPR-W 2020), an EXTENSION without a counterpart in the reference, in
the shape of `rise_videos.RiseVideo` with the arguments of `grad_cam_videos.GradCamVideo`.

`ScoreCamVideo(model, ['Mixed_5c'], ...)(clip, index)` returns `(map float32 [T,H,W], output [1,K])`: every channel of
the target layer is normalised to [0, 1], expanded to the clip with the bilinear + Gaussian map of the spacetime search
(`sigma` input pixels) and used as a mask on the input -- `perturb='freeze'` freezes the pixels the channel does not
fire on (the project's perturbation), `'blank'` multiplies them towards a zero baseline (the paper's form) -- and the
channel is weighted by what the masked clip scores above the fully perturbed one (`weights='increase'`) or by the
softmax of those (`'softmax'`, the paper's form).  The map is relu(sum_k w_k A_k), resized and normalised as the
Grad-CAM of the same layer.  No gradient is taken: one forward pass per channel, all through the HIP plan
(csrc/scorecam_ops.hip normalises, stages the masked clips and reduces); nothing falls back to PyTorch.
`channels=(first, count)` restricts the call to a window of the layer's channels.  The target layers are named as
`GradCamVideo` names them: an I3D endpoint, or 'clstm' / 'cell<i>' with `archType="CLSTM"`.
"""
import numpy as np

import ivf_lib as L
from grad_cam_videos import _arch, _clstm_layer, _one_target, _unwrap


class ScoreCamVideo:
    def __init__(self, model, target_layer_names, class_dict=None, use_cuda=True, input_spatial_size=224,
                 normalizePerFrame=False, weights="increase", perturb="freeze", sigma=None, channels=None,
                 archType="I3D"):
        self.model = _unwrap(model)
        self.archType = archType
        self.cuda = use_cuda
        self.class_dict = class_dict
        self.target_layers = target_layer_names
        self.normalizePerFrame = normalizePerFrame
        if isinstance(input_spatial_size, int):
            self.input_spatial_size = (input_spatial_size, input_spatial_size)
        elif len(input_spatial_size) == 1:
            self.input_spatial_size = (input_spatial_size[0], input_spatial_size[0])
        else:
            self.input_spatial_size = tuple(input_spatial_size)
        self.weights, self.perturb, self.sigma, self.channels = weights, perturb, sigma, channels
        self.last = None                # the engine's whole result dict of the last call (device tensors)
        if self.cuda:
            self.model = self.model.cuda()

    def __call__(self, input, index=None):
        _arch(self.archType)
        layer = _one_target(self.target_layers)
        if self.archType == "CLSTM":
            layer = _clstm_layer(self.model, layer)
        x = input.cuda() if self.cuda else input
        L.require_gpu(x)
        if x.shape[0] != 1:
            raise L.IvfError("ScoreCamVideo takes one clip [1,C,T,H,W], as GradCamVideo does")
        try:
            rows = 32 if self.channels is None else int(self.channels[1]) + 1
        except (TypeError, ValueError, IndexError):
            raise L.IvfError(f"channels must be (first, count), got {self.channels!r}")
        eng = self.model._engine_for(x, min_batch=max(1, min(32, rows)))    # the channel rows of one clip fill the plan
        output = eng.forward(x)
        target = [int(index)] if index is not None else eng.argmax(output)
        width, height = self.input_spatial_size             # cv2 dsize order, as GradCamVideo
        self.last = eng.scorecam(x, target, layer=layer, weights=self.weights, perturb=self.perturb, sigma=self.sigma,
                                 channels=self.channels, per_frame=bool(self.normalizePerFrame), out_hw=(height, width))
        return self.last["scorecam_map"][0].cpu().numpy().astype(np.float32), output
