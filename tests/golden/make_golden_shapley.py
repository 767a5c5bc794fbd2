#!/usr/bin/env python3
"""Generate tests/golden/shapley.npz: the 36 Shapley rows of 4 permutations on the REFERENCE's I3D model on CPU.

Needs the reference tree that make_golden.py puts on sys.path, so it runs where that tree is, never in a test:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_shapley.py

Shapley value sampling has no counterpart in the reference.  What is pinned here is the reference's own
`I3D_doubled.Model` with the recipe weights and the S16 recipe clip of rise.npz, under the torch restatement of the
expand (M = A_H S A_W^T, tests/stmask_refs.py) and of the per-pixel freeze of DESIGN section 11, on the explicit
per-frame S of each prefix of each of the 4 hash permutations (tests/shap_refs.py: seed 1234, antithetic, grid
(2, 2, 2), sigma 0: 4 x 9 rows) -- all in float32 -- and the fp64 estimator of shap_refs on those scores.
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
import shap_refs as SH                                   # noqa: E402
import stmask_refs as SR                                 # noqa: E402

R = G.R
CLIP, GRID, SIGMA, N, SEED, ANTI = 21, (2, 2, 2), 0.0, 4, 1234, True


def main():
    model = G._i3d(False)
    for p in model.parameters():
        p.requires_grad_(False)
    x = torch.from_numpy(R.clip(CLIP))[None]
    b, C, T, H, W = x.shape
    gt, gh, gw = GRID
    P = gt * gh * gw
    AH, AW = SR.axis_weights(H, gh, SIGMA), SR.axis_weights(W, gw, SIGMA)
    rk = SH.ranks(SEED, N, P, ANTI)
    rows = np.arange(N * (P + 1))
    S_all = torch.from_numpy(SH.frame_masks(SH.row_masks(rk, GRID, rows), T))            # [N (P+1),T,gh,gw]
    with torch.no_grad():
        probs = model(x)
        target = int(torch.argmax(probs[0]))
        scores = []
        for r in rows:
            M = AH @ S_all[r:r + 1] @ AW.t()                               # [1,T,H,W]
            frames = [x[:, :, 0]]
            for u in range(1, T):
                mu = M[:, u].unsqueeze(1)
                frames.append((1 - mu) * x[:, :, u] + mu * frames[-1])
            scores.append(float(model(torch.stack(frames, dim=2))[0, target]))
            print('  row', r, scores[-1], flush=True)
    scores = np.array(scores, np.float32).reshape(N, P + 1)
    orig = np.float32(probs[0, target])
    ref = SH.reduce_ref(scores[None], rk)
    G.save('shapley', clip=np.int64(CLIP), grid=np.array(GRID), sigma=np.float32(SIGMA), n=np.int64(N),
           seed=np.int64(SEED), antithetic=np.int64(ANTI), target=np.int64(target), orig=orig, scores=scores,
           ranks=rk.astype(np.int64), cells=ref["cells"][0].reshape(GRID), stderr=ref["stderr"][0].reshape(GRID),
           count=ref["count"][0].reshape(GRID), total=np.float64(ref["total"][0]))


if __name__ == '__main__':
    main()
