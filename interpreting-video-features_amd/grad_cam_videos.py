"""Drop-in for video_features_pytorch/grad_cam_videos.py (+ the names it re-exports
from the vendored pytorch-grad-cam/grad-cam.py via `from grad_cam import *`).

`GradCamVideo(model, ['Mixed_5c'], ...)(clip, index)` returns the same
`(cam_vid float32 [T,H,W], output [1,K])` pair, computed by the HIP plan: forward
to Mixed_5c, head backward from the (post-softmax) class score, channel-mean
weights, weighted sum + ReLU, bilinear resize, repeat, min/max normalise
(csrc/pool_head.hip; reference grad_cam_videos.py:64-142).

`archType="CLSTM"` (models.CLSTM_4.Model, csrc/convlstm.hip) takes two kinds of target layer name:
`['clstm']` is the reference's branch (grad-cam.py:33-49; the name it tests, `firstCLSTMLayer`, is not an
attribute of CLSTM_4.Model, whose ConvLSTM module is called `clstm`): the top layer's outputs at the effective
steps, each map repeated `T // n` times.  `['cell0']`, `['cell1']`, ... is an EXTENSION without a counterpart
in the reference: that layer's pooled output at every step, with the gradient through the layers above and
their recurrences, one map per frame.
"""
import re

import numpy as np
import torch

import ivf_lib as L


def _unwrap(model):
    return model.module if hasattr(model, "module") and not hasattr(model, "_engine_for") else model


def _one_target(target_layers):
    """Any ONE endpoint of the model may be the target layer.  With several, the reference pairs
    `features[-1]` (the LAST target in forward order) with `gradients[-1]` (the hook that fired last in the
    backward pass, i.e. the FIRST target): activations and gradients of different layers -- refused."""
    if len(target_layers) != 1:
        raise L.IvfError("GradCamVideo takes exactly one target layer (the reference mixes the activations of "
                         "the last target with the gradients of the first when given several)")
    return target_layers[0]


def _clstm_layer(model, name):
    """'clstm' -> None (the reference's stack), 'cell<i>' -> i (per-frame maps of layer i)."""
    if name == "clstm":
        return None
    m = re.fullmatch(r"cell(\d+)", str(name))
    if m is None or int(m.group(1)) >= model.lstm_layers:
        raise L.IvfError(f"'{name}' is not a Grad-CAM target of the ConvLSTM: 'clstm' or 'cell0' .. "
                         f"'cell{model.lstm_layers - 1}'")
    return int(m.group(1))


def _arch(archType):
    if archType not in ("I3D", "CLSTM"):
        raise L.IvfError(f"archType must be 'I3D' or 'CLSTM', got {archType!r}")
    return archType


class FeatureExtractor():
    """pytorch-grad-cam/grad-cam.py:11-54: activations of the target layers and the
    output of the last feature module.  Gradients are produced by the HIP head
    backward (no autograd hooks)."""

    def __init__(self, model, target_layers, archType="I3D"):
        self.model = _unwrap(model)
        self.archType = archType
        self.target_layers = target_layers
        self.gradients = []

    def save_gradient(self, grad):
        self.gradients.append(grad)

    def __call__(self, x):
        _arch(self.archType)
        name = _one_target(self.target_layers)
        self.gradients = []
        eng = self.model._engine_for(x)
        if self.archType == "CLSTM":
            # torch.stack(x[0]) of grad-cam.py:43-49: [n, B, hid, h, w]; the gradient of the predicted class's
            # score with respect to it is kept where the reference's hook would put it
            raw = eng.gradcam_raw(x, None, layer=_clstm_layer(self.model, name))
            self.gradients = [raw["grad"].transpose(0, 1).contiguous()]
            return [raw["feat"].transpose(0, 1).contiguous()], raw["probs"]
        eng.forward(x)
        acts = [eng.endpoint(t, x.shape[0]) for t in self.target_layers]
        return acts, eng.endpoint('Mixed_5c', x.shape[0])


class ModelOutputs():
    """pytorch-grad-cam/grad-cam.py:56-71 (2-D image models) -- name kept for import
    compatibility; the 2-D VGG demo path is outside the video saliency path."""

    def __init__(self, model, target_layers):
        self.model = model
        self.target_layers = target_layers

    def get_gradients(self):
        return self.feature_extractor.gradients

    def __call__(self, x):
        raise L.IvfError("ModelOutputs (2-D pytorch-grad-cam) is not part of the video path; use ModelOutputsVideo")


class ModelOutputsVideo(ModelOutputs):
    """grad_cam_videos.py:13-43."""

    def __init__(self, model, target_layers, archType):
        self.model = _unwrap(model)
        self.archType = archType
        self.feature_extractor = FeatureExtractor(self.model, target_layers, archType)

    def __call__(self, x):
        target_activations, feat = self.feature_extractor(x)
        if self.archType == "CLSTM":     # the model's own output, grad_cam_videos.py:27-43
            return target_activations, feat
        eng = self.model._engine_for(x)
        output = eng.forward(x)          # head of grad_cam_videos.py:30-41 (avg-pool, logits, softmax)
        return target_activations, output


class GradCam:
    """pytorch-grad-cam/grad-cam.py:96-145 (2-D) -- importable, not on the video path."""

    def __init__(self, model, target_layer_names, use_cuda):
        self.model = model
        self.cuda = use_cuda

    def forward(self, input):
        return self.model(input)

    def __call__(self, input, index=None):
        raise L.IvfError("GradCam (2-D) is not part of the video path; use GradCamVideo")


class GradCamVideo(GradCam):
    """grad_cam_videos.py:46-142.  `kind` (an EXTENSION) selects another member of the activation-map
    family on the same target layer: 'gradcam++', 'xgradcam', 'hirescam' or 'layercam'; the default 'gradcam' is the
    reference's map on the reference's call path."""

    def __init__(self, model, target_layer_names, class_dict, use_cuda,
                 input_spatial_size=224, normalizePerFrame=False, archType="I3D", kind="gradcam"):
        L.cam_kind_ids([kind])                              # an unknown kind is refused here, naming the five
        self.kind = kind
        self.model = _unwrap(model)
        self.archType = archType
        self.cuda = use_cuda
        self.normalizePerFrame = normalizePerFrame
        # the reference calls len() on this (grad_cam_videos.py:54), which fails for the
        # int default; accept an int or a 1-/2-sequence (width, height)
        if isinstance(input_spatial_size, int):
            self.input_spatial_size = (input_spatial_size, input_spatial_size)
        elif len(input_spatial_size) == 1:
            self.input_spatial_size = (input_spatial_size[0], input_spatial_size[0])
        else:
            self.input_spatial_size = tuple(input_spatial_size)
        self.class_dict = class_dict
        if self.cuda:
            self.model = self.model.cuda()
        self.extractor = ModelOutputsVideo(self.model, target_layer_names, self.archType)

    def __call__(self, input, index=None):
        _arch(self.archType)
        layer = _one_target(self.extractor.feature_extractor.target_layers)
        if self.archType == "CLSTM":
            layer = _clstm_layer(self.model, layer)
        x = input.cuda() if self.cuda else input
        L.require_gpu(x)
        if x.shape[0] != 1:
            raise L.IvfError("GradCamVideo takes one clip [1,C,T,H,W], as the reference does (smth:264)")
        eng = self.model._engine_for(x)
        target = None
        if index is not None:
            target = [int(index)]                           # grad_cam_videos.py:69-72
        width, height = self.input_spatial_size             # cv2 dsize order, grad_cam_videos.py:119-120
        if self.kind == "gradcam":
            cam, output = eng.gradcam(x, target, per_frame=bool(self.normalizePerFrame), out_hw=(height, width),
                                      layer=layer)
        else:
            cams, output = eng.cam(x, target, kinds=(self.kind,), per_frame=bool(self.normalizePerFrame),
                                   out_hw=(height, width), layer=layer)
            cam = cams[self.kind]
        cam_vid = cam[0].cpu().numpy().astype(np.float32)
        return cam_vid, output
