#!/usr/bin/env python3
"""Generate tests/golden/rise.npz: scores of 16 RISE masks on the REFERENCE's I3D model on CPU.

Run in the build container only (needs the reference tree, which never travels to the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rise.py

RISE has no counterpart in the reference.  What is pinned here is the reference's own `I3D_doubled.Model` with the
recipe weights and the S16 recipe clip of box.npz, under the torch restatement of the expand (M = A_H S A_W^T,
tests/stmask_refs.py) and of the per-pixel freeze of DESIGN section 11, on the explicit per-frame S of each of the 16 hash
masks (tests/rise_refs.py: seed 1234, p 0.5, grid (2, 2, 2), sigma 0) -- all in float32 -- and the fp64 estimator of
rise_refs on those scores.
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
import rise_refs as RR                                   # noqa: E402
import stmask_refs as SR                                 # noqa: E402

R = G.R
CLIP, GRID, SIGMA, N, P, SEED = 21, (2, 2, 2), 0.0, 16, 0.5, 1234


def main():
    model = G._i3d(False)
    for p in model.parameters():
        p.requires_grad_(False)
    x = torch.from_numpy(R.clip(CLIP))[None]
    b, C, T, H, W = x.shape
    gt, gh, gw = GRID
    AH, AW = SR.axis_weights(H, gh, SIGMA), SR.axis_weights(W, gw, SIGMA)
    S_all = torch.from_numpy(RR.frame_masks(RR.masks(SEED, P, N, GRID), T))          # [N,T,gh,gw]
    with torch.no_grad():
        probs = model(x)
        target = int(torch.argmax(probs[0]))
        scores = []
        for k in range(N):
            M = AH @ S_all[k:k + 1] @ AW.t()                               # [1,T,H,W]
            frames = [x[:, :, 0]]
            for u in range(1, T):
                mu = M[:, u].unsqueeze(1)
                frames.append((1 - mu) * x[:, :, u] + mu * frames[-1])
            scores.append(float(model(torch.stack(frames, dim=2))[0, target]))
            print('  mask', k, scores[-1], flush=True)
    scores = np.array(scores, np.float32)
    orig = np.float32(probs[0, target])
    cells, count, mean_drop, _ = RR.reduce_ref(scores[None], [orig], SEED, P, GRID)
    G.save('rise', clip=np.int64(CLIP), grid=np.array(GRID), sigma=np.float32(SIGMA), n=np.int64(N), p=np.float64(P),
           seed=np.int64(SEED), target=np.int64(target), orig=orig, scores=scores, cells=cells[0].astype(np.float64),
           count=count[0], mean_drop=np.float64(mean_drop[0]))


if __name__ == '__main__':
    main()
