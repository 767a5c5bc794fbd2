#!/usr/bin/env python3
"""Generate tests/golden/scorecam.npz: Score-CAM of 24 channels of Mixed_5c on the REFERENCE's I3D model on CPU.

Run in the build container only (needs the reference tree, which never travels to the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_scorecam.py

Score-CAM has no counterpart in the reference.  What is pinned here is the reference's own `I3D_doubled.Model` with the
recipe weights and the S16 recipe clip of rise.npz: its Mixed_5c activations (a forward hook), the float32 normalise of
tests/scorecam_refs.py on channels [100, 124), the scores of the 24 channel rows and the baseline row under the torch
restatement of the expand (M = A_H S A_W^T, tests/stmask_refs.py, sigma 0) and of the per-pixel freeze of DESIGN section 11
on the explicit per-frame S of each row -- all in float32 -- and on those scores the 'increase' weights (one fp32
subtraction), the fp64 softmax weights and the fp64 cam of scorecam_refs under either (the 'increase' weights are
signed, and on this clip their map is 0 everywhere after the relu; the 'softmax' map is the one with a scale).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden as G                                  # noqa: E402  (reference modules on sys.path)

sys.path.insert(0, os.path.dirname(HERE))
import scorecam_refs as SC                               # noqa: E402
import stmask_refs as SR                                 # noqa: E402

R = G.R
CLIP, LAYER, FIRST, COUNT, SIGMA = 21, 'Mixed_5c', 100, 24, 0.0


def main():
    model = G._i3d(False)
    for p in model.parameters():
        p.requires_grad_(False)
    x = torch.from_numpy(R.clip(CLIP))[None]
    b, C, T, H, W = x.shape
    kept = {}
    hook = model._modules[LAYER].register_forward_hook(lambda m, i, o: kept.__setitem__('A', o.detach().clone()))
    with torch.no_grad():
        probs = model(x)
    hook.remove()
    target = int(torch.argmax(probs[0]))
    A = kept['A'][:, FIRST:FIRST + COUNT].float().numpy()                      # [1,24,gt,gh,gw]
    gt, gh, gw = A.shape[2:]
    lo, hi, valid, F = SC.normalise(A)
    assert int(valid.sum()) >= 16, f"only {int(valid.sum())} of the {COUNT} channels from {FIRST} are valid: move the window"
    AH, AW = SR.axis_weights(H, gh, SIGMA), SR.axis_weights(W, gw, SIGMA)
    S_all = torch.from_numpy(SC.frame_planes(F[0], T))                         # [24,T,gh,gw]
    scores = []
    with torch.no_grad():
        for k in range(COUNT + 1):
            if k < COUNT:
                M = AH @ S_all[k:k + 1] @ AW.t()                               # [1,T,H,W]
                frames = [x[:, :, 0]]
                for u in range(1, T):
                    mu = M[:, u].unsqueeze(1)
                    frames.append((1 - mu) * x[:, :, u] + mu * frames[-1])
                row = torch.stack(frames, dim=2)
            else:
                row = x[:, :, :1].expand(-1, -1, T, -1, -1).contiguous()       # the baseline row: every frame = frame 0
            scores.append(float(model(row)[0, target]))
            print('  row', k, scores[-1], flush=True)
    scores = np.array(scores, np.float32)[None]
    w_inc = SC.weights_increase(scores, valid)
    w_soft, _ = SC.weights_softmax(scores, valid)
    cam_inc, _ = SC.cam_ref(w_inc, A)            # signed weights: may be 0 everywhere after the relu
    cam_soft, _ = SC.cam_ref(w_soft, A)          # positive weights on post-ReLU activations: positive
    assert len(np.unique(scores)) > 1 and cam_soft.max() > 0
    G.save('scorecam', clip=np.int64(CLIP), first=np.int64(FIRST), count=np.int64(COUNT), sigma=np.float32(SIGMA),
           target=np.int64(target), orig=np.float32(probs[0, target]), A=A[0].astype(np.float32), lo=lo[0], hi=hi[0],
           valid=valid[0], F=F[0].astype(np.float32), scores=scores[0], w_increase=w_inc[0],
           w_softmax=w_soft[0].astype(np.float64), cam_increase=cam_inc[0].astype(np.float64),
           cam_softmax=cam_soft[0].astype(np.float64))


if __name__ == '__main__':
    main()
