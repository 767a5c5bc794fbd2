#!/usr/bin/env python3
"""Generate tests/golden/box.npz: scores of a dozen one-box candidates (maskType='stcombi') on the REFERENCE's I3D
model on CPU.

Run in the build container only (needs the reference tree, which never travels to the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_box.py

The one-box search has no counterpart in the reference.  What is pinned here is the reference's own
`I3D_doubled.Model` with the recipe weights and the S16 recipe clip of blob.npz, under the torch restatement of the
expand (M = A_H S A_W^T, tests/stmask_refs.py) and of the per-pixel freeze of DESIGN section 11, on the explicit binary S
of each listed candidate -- all in float32.  Grid 2 x 2, sigma 0, candidates (a, L, i0, bh, j0, bw) within max_len 2 and
max_box (2, 2).
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
import stmask_refs as SR                                 # noqa: E402

R = G.R
CLIP, GRID, SIGMA, MAX_LEN, MAX_BOX = 21, (2, 2), 0.0, 2, (2, 2)
CANDIDATES = [(0, 1, 0, 1, 0, 1), (0, 2, 0, 2, 0, 2), (1, 1, 0, 1, 0, 1), (1, 1, 1, 1, 1, 1), (5, 1, 0, 1, 1, 1),
              (5, 2, 1, 1, 0, 1), (8, 2, 0, 2, 0, 1), (8, 2, 0, 1, 0, 2), (11, 1, 0, 2, 0, 2), (14, 2, 0, 2, 0, 2),
              (15, 1, 1, 1, 0, 2), (3, 2, 0, 2, 1, 1)]


def main():
    model = G._i3d(False)
    for p in model.parameters():
        p.requires_grad_(False)
    x = torch.from_numpy(R.clip(CLIP))[None]
    b, C, T, H, W = x.shape
    gh, gw = GRID
    AH, AW = SR.axis_weights(H, gh, SIGMA), SR.axis_weights(W, gw, SIGMA)
    with torch.no_grad():
        probs = model(x)
        target = int(torch.argmax(probs[0]))
        scores = []
        for (a, L, i0, bh, j0, bw) in CANDIDATES:
            S = torch.zeros(1, T, gh, gw)
            S[0, a:a + L, i0:i0 + bh, j0:j0 + bw] = 1.0
            M = AH @ S @ AW.t()                                        # [1,T,H,W]
            frames = [x[:, :, 0]]
            for u in range(1, T):
                mu = M[:, u].unsqueeze(1)
                frames.append((1 - mu) * x[:, :, u] + mu * frames[-1])
            scores.append(float(model(torch.stack(frames, dim=2))[0, target]))
            print('  candidate', (a, L, i0, bh, j0, bw), scores[-1], flush=True)
    G.save('box', clip=np.int64(CLIP), grid=np.array(GRID), sigma=np.float32(SIGMA), max_len=np.int64(MAX_LEN),
           max_box=np.array(MAX_BOX), target=np.int64(target), orig=np.float32(probs[0, target]),
           candidates=np.array(CANDIDATES, np.int64), scores=np.array(scores, np.float32))


if __name__ == '__main__':
    main()
