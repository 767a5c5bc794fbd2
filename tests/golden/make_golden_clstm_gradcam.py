#!/usr/bin/env python3
"""Generate tests/golden/clstm_gradcam.npz: Grad-CAM of the ConvLSTM (archType='CLSTM') from the REFERENCE's
models.CLSTM_4.Model and torch autograd on the CPU.

Run in the build container only (needs the reference tree, which never travels to the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_clstm_gradcam.py

The reference's GradCamVideo.__call__ (grad_cam_videos.py:64-142) does all the arithmetic: backward from the class
score, channel means, weighted sum, ReLU, resize (cv2.resize bound to oracle.gradcam_ref.resize_bilinear, as in
make_golden.py), repeat, normalisation.  Only its feature extractor cannot run for this model (it tests attribute
names CLSTM_4.Model lacks), so the extractor object is replaced by `Extractor` below, which hands over what that
branch builds (grad-cam.py:43-49): the stack `[n, B, hid, h, w]` of the chosen pooled outputs and, after the
backward, the gradient autograd left on them.  A forward hook on `model.clstm.mp` sees every pooled output; it
fires T * layers times, step-major, layer-minor.

  target 'clstm'   : top layer at the effective steps (the reference's branch)
  target 'cell<i>' : layer i at every step (extension; the gradient runs through the layers above)

Geometry: KTH, 3 x 32 x 120 x 160, 2 layers, hidden 4, stride 2, effective steps 7/15/23/31, recipe weights
'clstm3', clip 7, class = argmax.  With use_entire_seq the endFC tensors are the recipe's at four times the width
(`clstm_state_dict(fc_mult=4)`, same tag), so the tests rebuild them and nothing of them is stored.
Every normalised block must have a positive maximum (0/0 = NaN in the reference otherwise): asserted here.

Stored per case `e{0,1}_s{0,1}_{clstm,cell0,cell1}`: probs, index, w, raw cam (cell0: [::2, ::2, ::2]), the final
maps for normalizePerFrame True (`_pf1`, [:, ::8, ::8]) and False (`_pf0`, [::4, ::8, ::8]); for the top layer also
the gradient stack at the effective steps, and once (`cell1_feat`) the top layer's features at every step.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden as G                                  # noqa: E402  (reference modules on sys.path, cv2 bound)

R = G.R
T, LAYERS, EFF = 32, 2, [7, 15, 23, 31]
W_OUT, H_OUT = 160, 120


class Extractor:
    """Stands where ModelOutputsVideo stands in GradCamVideo: __call__ -> ([stack], output), get_gradients()."""

    def __init__(self, model, name):
        self.model, self.name = model, name

    def __call__(self, x):
        outs = []
        h = self.model.clstm.mp.register_forward_hook(lambda mod, inp, out: outs.append(out))
        y = self.model(x)
        h.remove()
        assert len(outs) == T * LAYERS
        if self.name == 'clstm':
            self.sel = [outs[t * LAYERS + LAYERS - 1] for t in EFF]
        else:
            self.sel = outs[int(self.name[4:])::LAYERS]
        for o in self.sel:
            o.retain_grad()
        return [torch.stack(self.sel).detach()], y

    def get_gradients(self):
        return [torch.stack([o.grad if o.grad is not None else torch.zeros_like(o) for o in self.sel])]


def model(entire, softmax):
    m = G.CLSTM_4.Model(num_classes=6, nb_lstm_units=4, channels=3, conv_kernel_size=(5, 5), lstm_layers=LAYERS,
                        step=T, image_size=(160, 120), conv_stride=2, effective_step=EFF, use_entire_seq=entire,
                        add_softmax=softmax).eval()
    m.load_state_dict(R.to_torch(R.clstm_state_dict(channels=3, tag='clstm3', fc_mult=4 if entire else 1)))
    return m


def main():
    out = {}
    x = torch.from_numpy(R.clip(7, 3, T, 120, 160) / 255.0)[None].float()
    for entire in (0, 1):
        for softmax in (0, 1):
            m = model(bool(entire), bool(softmax))
            for name in ('clstm', 'cell0', 'cell1'):
                key = f'e{entire}_s{softmax}_{name}'
                for pf in (1, 0):
                    gc = G.ref_gc.GradCamVideo(model=m, target_layer_names=[name], class_dict=None, use_cuda=False,
                                               input_spatial_size=(W_OUT, H_OUT), normalizePerFrame=bool(pf),
                                               archType="CLSTM")
                    gc.extractor = ex = Extractor(m, name)
                    vid, y = gc(x, None)
                    feat = torch.stack(ex.sel).detach().numpy()[:, 0]          # [n, hid, h, w]
                    grad = ex.get_gradients()[0].numpy()[:, 0]
                    n = feat.shape[0]
                    assert vid.shape == (n * (T // n), H_OUT, W_OUT) and np.isfinite(vid).all()
                    # the project's CPU restatement must agree with the reference to the bit
                    vid2, w, cam = G.gradcam_ref.cam_from_activations(
                        feat.transpose(1, 0, 2, 3), grad.transpose(1, 0, 2, 3), T, W_OUT, H_OUT, bool(pf))
                    assert np.array_equal(vid, vid2)
                    # every normalised block has a positive maximum (else the reference divides 0 by 0)
                    blocks = cam if pf else cam[None]
                    assert all(float(b.max()) > 0 for b in blocks), key
                    out[f'{key}_pf{pf}'] = vid[:, ::8, ::8] if pf else vid[::4, ::8, ::8]
                out[f'{key}_probs'] = y.detach().numpy()
                out[f'{key}_index'] = np.array(int(np.argmax(y.detach().numpy())))
                out[f'{key}_w'] = w
                out[f'{key}_cam'] = cam[::2, ::2, ::2] if name == 'cell0' else cam
                if name == 'clstm':
                    out[f'{key}_grad'] = grad
                    assert (np.abs(grad).reshape(n, -1).max(axis=1) > 0).sum() == (n if entire else 1)
                if name == 'cell0':
                    assert (np.abs(grad).reshape(n, -1).max(axis=1) > 0).all()
                if name == 'cell1' and softmax == 0 and entire == 0:
                    out['cell1_feat'] = feat            # the features depend on neither the head nor the target
    G.save('clstm_gradcam', **out)


if __name__ == '__main__':
    main()
