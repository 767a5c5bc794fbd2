#!/usr/bin/env python3
"""Generate tests/golden/curves.npz: the 2 x 9 deletion / insertion rows on the REFERENCE's I3D model on CPU.

Needs the reference tree that make_golden.py puts on sys.path, so it runs where that tree is, never in a test:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_curves.py

Deletion and insertion curves have no counterpart in the reference.  What is pinned here is the reference's own
`I3D_doubled.Model` with the recipe weights and the S16 recipe clip of shapley.npz, under the torch restatement of the
expand (M = A_H S A_W^T, tests/stmask_refs.py) and of the per-pixel freeze of DESIGN section 11, on the explicit
per-frame S of each row of both curves at step 1 (tests/curve_refs.py: grid (2, 2, 2), sigma 0, the cells ranked most
relevant first by the `cells` of shapley.npz: 2 x 9 rows, 18 forward passes) -- all in float32 -- and the fp64
reduction of curve_refs on those scores at step 1 and at step 3 (whose rows 0, 3, 6, 8 are a subset of the step-1 rows).
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
import curve_refs as CR                                  # noqa: E402
import stmask_refs as SR                                 # noqa: E402

R = G.R
CLIP, GRID, SIGMA = 21, (2, 2, 2), 0.0


def main():
    shap = dict(np.load(os.path.join(HERE, 'shapley.npz')))
    assert int(shap['clip']) == CLIP and tuple(int(v) for v in shap['grid']) == GRID and float(shap['sigma']) == SIGMA
    attr = shap['cells'].astype(np.float32)                  # what the device is given: fp32 cells [gt,gh,gw]
    model = G._i3d(False)
    for p in model.parameters():
        p.requires_grad_(False)
    x = torch.from_numpy(R.clip(CLIP))[None]
    b, C, T, H, W = x.shape
    gt, gh, gw = GRID
    P = gt * gh * gw
    AH, AW = SR.axis_weights(H, gh, SIGMA), SR.axis_weights(W, gw, SIGMA)
    rk = CR.ranks(attr.reshape(1, P), 0)
    rows = CR.row_list(1, P, 1, 3)
    S_all = torch.from_numpy(CR.frame_masks(CR.row_masks(rk, GRID, rows), T))            # [2 (P+1),T,gh,gw]
    with torch.no_grad():
        probs = model(x)
        target = int(torch.argmax(probs[0]))
        assert target == int(shap['target'])
        scores = []
        for r in range(len(rows)):
            M = AH @ S_all[r:r + 1] @ AW.t()                               # [1,T,H,W]
            frames = [x[:, :, 0]]
            for u in range(1, T):
                mu = M[:, u].unsqueeze(1)
                frames.append((1 - mu) * x[:, :, u] + mu * frames[-1])
            scores.append(float(model(torch.stack(frames, dim=2))[0, target]))
            print('  row', rows[r], scores[-1], flush=True)
    scores = np.array(scores, np.float32).reshape(2, P + 1)
    r1 = CR.auc_ref(scores[None], P, 1, 3)
    sub = CR.thresholds(P, 3)
    r3 = CR.auc_ref(scores[None][:, :, sub], P, 3, 3)
    G.save('curves', clip=np.int64(CLIP), grid=np.array(GRID), sigma=np.float32(SIGMA), target=np.int64(target),
           orig=np.float32(probs[0, target]), attr=attr, ranks=rk[0].astype(np.int64), scores=scores,
           auc_step1=r1["auc"][0], auc_norm_step1=r1["auc_norm"][0], step3_rows=sub.astype(np.int64),
           auc_step3=r3["auc"][0], auc_norm_step3=r3["auc_norm"][0])


if __name__ == '__main__':
    main()
