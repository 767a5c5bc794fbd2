#!/usr/bin/env python3
"""Generate tests/golden/blob.npz: the exhaustive one-blob temporal mask search (maskType='combi') restated on the
REFERENCE modules on CPU.

Run in the build container only (needs the reference tree, which never travels to the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_blob.py

Every one-blob binary mask m_{a,L} (1 on [a, a+L), 1 <= L <= max_len, canonical order L then a) is applied with the
reference's own mask.perturb_sequence and scored by the reference model; J = lam1*sum(m) + lam2*calc_tv_norm(m,3,3)
+ score is evaluated in fp32 with the reference's calc_tv_norm (the loss of smth:198-207 at a binary mask).  Weights
and clips come from ivf_recipe with the seeds of search.npz / search_long.npz.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden as G                                  # noqa: E402  (reference modules on sys.path)

R = G.R
ref_mask = G.ref_mask


def candidates(T, max_len):
    return [(a, L) for L in range(1, max_len + 1) for a in range(T - L + 1)]


def blob_mask(T, a, L):
    m = torch.zeros(T)
    m[a:a + L] = 1
    return m


def select(scores, J, orig, full, cands, threshold=0.9):
    """best = argmin J (ties: smaller L, then smaller a -- the canonical order); minimal = smallest L with some
    r >= threshold, largest r within it, then smaller a; (-1, -1) if none (or r NaN)."""
    best = cands[int(np.argmin(J))]            # np.argmin returns the first minimum = canonical tie rule
    r = (np.float32(orig) - scores) / (np.float32(orig) - np.float32(full))
    minimal = (-1, -1)
    for L in sorted({c[1] for c in cands}):
        idx = [k for k, c in enumerate(cands) if c[1] == L and r[k] >= threshold]
        if idx:
            k = max(idx, key=lambda k: (r[k], -cands[k][0]))
            minimal = cands[k]
            break
    return best, minimal


def run_case(out, tag, model, x, lam1, lam2, modes, max_len, chunk=8):
    T = x.shape[2]
    with torch.no_grad():
        probs = model(x)[0]
        target = int(torch.argmax(probs))
        orig = float(probs[target])
        full = float(model(x[:, :, :1].expand_as(x).contiguous())[0, target])   # mask.py:123-128
    cands = candidates(T, max_len)
    out[f'{tag}_target'] = np.array(target)
    out[f'{tag}_orig'] = np.array(orig, dtype=np.float32)
    out[f'{tag}_full'] = np.array(full, dtype=np.float32)
    out[f'{tag}_max_len'] = np.array(max_len)
    out[f'{tag}_lam'] = np.array([lam1, lam2], dtype=np.float32)
    for mode in modes:
        scores = []
        for s in range(0, len(cands), chunk):
            part = cands[s:s + chunk]
            with torch.no_grad():
                p = torch.cat([ref_mask.perturb_sequence(x, blob_mask(T, a, L), perturbation_type=mode)
                               for a, L in part])
                scores += model(p)[:, target].tolist()
            print(f'  {tag} {mode} {s + len(part)}/{len(cands)}', flush=True)
        scores = np.asarray(scores, dtype=np.float32)
        J = []
        for (a, L), sc in zip(cands, scores):
            m = blob_mask(T, a, L)
            l1 = lam1 * torch.sum(torch.abs(m))
            tv = lam2 * ref_mask.calc_tv_norm(m, p=3, q=3)
            J.append(float(l1 + tv + torch.tensor(sc)))
        J = np.asarray(J, dtype=np.float32)
        best, minimal = select(scores, J, orig, full, cands)
        out[f'{tag}_{mode}_scores'] = scores
        out[f'{tag}_{mode}_J'] = J
        out[f'{tag}_{mode}_best'] = np.array(best, dtype=np.int32)
        out[f'{tag}_{mode}_minimal'] = np.array(minimal, dtype=np.int32)
        print(f'  {tag} {mode}: best {best} J {J.min():.6f}, minimal {minimal}', flush=True)


def main():
    out = {}
    m = G._i3d(False)
    run_case(out, 's16', m, torch.from_numpy(R.clip(21))[None], 0.01, 0.02, ('freeze', 'reverse'), 16)
    del m
    m = G._i3d(True, T=32)
    run_case(out, 'k32', m, torch.from_numpy(R.clip(23, 3, 32, 120, 160))[None], 0.02, 0.04, ('freeze',), 8)
    del m
    c = G._clstm(1)
    run_case(out, 'c1', c, torch.from_numpy(R.clip(3, 1, 32, 120, 160) / 255.0)[None], 0.02, 0.04,
             ('freeze', 'reverse'), 32, chunk=32)
    G.save('blob', **out)


if __name__ == '__main__':
    main()
