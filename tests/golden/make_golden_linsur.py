#!/usr/bin/env python3
"""Generate tests/golden/linsur.npz: 32 KernelSHAP rows, 32 LIME rows and the fully frozen row on the REFERENCE's I3D
model on CPU.

Needs the reference tree that make_golden.py puts on sys.path, so it runs where that tree is, never in a test:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_linsur.py

KernelSHAP and LIME have no counterpart in the reference.  What is pinned here is the reference's own
`I3D_doubled.Model` with the recipe weights and the S16 recipe clip of shapley.npz, under the torch restatement of the
expand (M = A_H S A_W^T, tests/stmask_refs.py) and of the per-pixel freeze of DESIGN section 11, on the explicit
per-frame S of each sample row (tests/linsur_refs.py: seed 1234, grid (2, 2, 2), sigma 0; KernelSHAP paired, LIME
p 0.5, width 0.25, ridge 1) -- all in float32 -- and the fp64 fits of linsur_refs on those scores.
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
import linsur_refs as LR                                 # noqa: E402
import rise_refs as RR                                   # noqa: E402
import stmask_refs as SR                                 # noqa: E402

R = G.R
CLIP, GRID, SIGMA, N, SEED, PROB, WIDTH, RIDGE = 21, (2, 2, 2), 0.0, 32, 1234, 0.5, 0.25, 1.0


def main():
    model = G._i3d(False)
    for p in model.parameters():
        p.requires_grad_(False)
    x = torch.from_numpy(R.clip(CLIP))[None]
    b, C, T, H, W = x.shape
    gt, gh, gw = GRID
    P = gt * gh * gw
    AH, AW = SR.axis_weights(H, gh, SIGMA), SR.axis_weights(W, gw, SIGMA)
    Zk, sizes = LR.kshap_rows(SEED, N, P, True)
    Zl = LR.lime_rows(SEED, RR.thresh(PROB), N, P)
    Z_all = np.concatenate([Zk, Zl, np.ones((1, P), bool)])                # 2 N + 1 rows
    S_all = torch.from_numpy(RR.frame_masks(Z_all.reshape(-1, gt, gh, gw).astype(np.float32), T))   # [2N+1,T,gh,gw]
    with torch.no_grad():
        probs = model(x)
        target = int(torch.argmax(probs[0]))
        scores = []
        for r in range(len(Z_all)):
            M = AH @ S_all[r:r + 1] @ AW.t()                               # [1,T,H,W]
            frames = [x[:, :, 0]]
            for u in range(1, T):
                mu = M[:, u].unsqueeze(1)
                frames.append((1 - mu) * x[:, :, u] + mu * frames[-1])
            scores.append(float(model(torch.stack(frames, dim=2))[0, target]))
            print('  row', r, scores[-1], flush=True)
    scores = np.array(scores, np.float32)
    orig = np.float32(probs[0, target])
    ks = np.concatenate([scores[:N], scores[-1:]])[None]                   # [1, N+1]
    ls = np.concatenate([scores[N:2 * N], scores[-1:]])[None]
    fk = LR.kshap_fit(Zk, ks, orig[None])
    wt = LR.lime_wtab(P, WIDTH)
    fl = LR.lime_fit(Zl, ls, orig[None], wt, RIDGE)
    assert not fk["singular"] and not fl["singular"]
    r2k = LR.r2_ref(Zk, fk["w"], ks, orig[None], fk["cells"].astype(np.float32), [0.0], fk["t"], fk["Wsum"])
    r2l = LR.r2_ref(Zl, fl["w"], ls, orig[None], fl["cells"].astype(np.float32), fl["intercept"].astype(np.float32),
                    fl["t"], fl["Wsum"])
    G.save('linsur', clip=np.int64(CLIP), grid=np.array(GRID), sigma=np.float32(SIGMA), n=np.int64(N),
           seed=np.int64(SEED), paired=np.int64(1), p=np.float64(PROB), width=np.float64(WIDTH), ridge=np.float64(RIDGE),
           target=np.int64(target), orig=orig, kshap_rows=Zk, kshap_sizes=sizes, lime_rows=Zl, kshap_scores=ks[0],
           lime_scores=ls[0], kshap_cells=fk["cells"][0].reshape(GRID), kshap_total=np.float64(fk["total"][0]),
           kshap_r2=np.float64(r2k[0]), lime_cells=fl["cells"][0].reshape(GRID),
           lime_intercept=np.float64(fl["intercept"][0]), lime_r2=np.float64(r2l[0]))


if __name__ == '__main__':
    main()
