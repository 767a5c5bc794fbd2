#!/usr/bin/env python3
"""Generate tests/golden/stmask.npz: six iterations of the spatio-temporal mask search (maskType='spacetime') on the
REFERENCE's I3D model on CPU.

Run in the build container only (needs the reference tree, which never travels to the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stmask.py

The spacetime search has no counterpart in the reference.  What is pinned here is the reference's own
`I3D_doubled.Model` with the recipe weights and clips of search.npz, under the torch restatement of the perturbation
and loss of DESIGN section 11 (tests/stmask_refs.py: axis matrices, per-pixel freeze, regulariser), differentiated by
torch autograd and stepped by torch.optim.Adam -- all in float32, as the reference's own loop runs.
2 clips, S16, grid 7x7, sigma 16, lam = (0.01, 0.02, 0.02), 6 iterations from init_mask('central') rows.
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
CLIPS, GRID, SIGMA, LAMS, N = (21, 7), (7, 7), 16.0, (0.01, 0.02, 0.02), 6


def central_init(model, x, target, T):
    """init_mask(mode='central') rows, as make_golden._ref_search restates it (mask.py:121-154)"""
    with torch.no_grad():
        full = model(x[:, :, :1].expand_as(x).contiguous())[0, target]
        orig = model(x)[0, target]
        for i in range(1, T // 2):
            nm = torch.ones(T)
            nm[:i] = 0
            nm[-i:] = 0
            c = model(G.ref_mask.perturb_sequence(x, nm, perturbation_type='freeze'))[0, target]
            if (orig - c) / (orig - full) < 0.9:
                break
    return torch.where(nm == 0, torch.tensor(-5.0), torch.tensor(5.0)), float(orig)


def main():
    model = G._i3d(False)
    for p in model.parameters():
        p.requires_grad_(False)
    x = torch.from_numpy(np.stack([R.clip(c) for c in CLIPS]))
    b, C, T, H, W = x.shape
    gh, gw = GRID
    with torch.no_grad():
        targets = torch.argmax(model(x), dim=1)
    rows, orig = zip(*[central_init(model, x[r:r + 1], int(targets[r]), T) for r in range(b)])
    rows = torch.stack(rows)
    AH, AW = SR.axis_weights(H, gh, SIGMA), SR.axis_weights(W, gw, SIGMA)
    raw = rows.view(b, T, 1, 1).expand(b, T, gh, gw).clone().requires_grad_()
    opt = torch.optim.Adam([raw], lr=0.2)
    traj = []
    for n in range(N):
        S = torch.sigmoid(raw)
        M = AH @ S @ AW.t()                                            # [b,T,H,W]
        frames = [x[:, :, 0]]
        for u in range(1, T):
            mu = M[:, u].unsqueeze(1)
            frames.append((1 - mu) * x[:, :, u] + mu * frames[-1])
        score = model(torch.stack(frames, dim=2))[torch.arange(b), targets]
        l1, tvt, tvs = SR.reg_terms64(S, LAMS)                         # float32 here: the dtype of S
        loss = l1 + tvt + tvs + score
        opt.zero_grad()
        loss.sum().backward()                                          # clips are independent in eval mode
        opt.step()
        traj.append(torch.stack([loss, l1, tvt, tvs, score], dim=1).detach().numpy())
        print('  iter', n, traj[-1].tolist(), flush=True)
    S = torch.sigmoid(raw.detach())
    time_mask = S.mean(dim=(2, 3))
    with torch.no_grad():
        rev = [float(model(G.ref_mask.perturb_sequence(x[r:r + 1], time_mask[r], perturbation_type='reverse'))[0, targets[r]])
               for r in range(b)]
    G.save('stmask', clips=np.array(CLIPS), grid=np.array(GRID), sigma=np.float32(SIGMA), lams=np.array(LAMS, np.float32),
           target=targets.numpy(), orig=np.array(orig, np.float32), init=rows.numpy(), traj=np.stack(traj).astype(np.float32),
           st_mask=S.numpy(), time_mask=time_mask.numpy(), freeze_score=traj[-1][:, 4], reverse_score=np.array(rev, np.float32))


if __name__ == '__main__':
    main()
