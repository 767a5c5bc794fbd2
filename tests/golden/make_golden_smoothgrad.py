#!/usr/bin/env python3
"""Generate tests/golden/smoothgrad.npz: SmoothGrad, SmoothGrad^2 and VarGrad by torch autograd on the
REFERENCE's own I3D_doubled.Model with the recipe weights.  Run where make_golden.py runs:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_smoothgrad.py

The method has no counterpart in the reference; what is pinned is the gradient of the reference's model at the noisy
points and the semantics (tests/sg_refs.py restates them, the noise included).  Clips 21 and 7, n = 8 samples,
level = 0.15, seed 0, target = the model's argmax on the clip.  The three maps are stored at make_golden.sample_idx
positions; the frame sums, sample scores, sigma and the moment totals whole.  Three legs, as make_golden_ig: fp32 / 8
threads (the fixture proper), fp64, and fp32 / 4 threads (another summation order inside torch's convolutions) -- the
distance between them is the noise floor the GPU gates are set against, and for var_map it IS the gate.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG          # noqa: E402  (binds the reference's modules and the recipe)
sys.path.append(os.path.dirname(HERE))
import sg_refs as SR              # noqa: E402

R = MG.R
CLIPS = SR.I3D_CLIPS
N, LEVEL, SEED = SR.I3D_N, SR.I3D_LEVEL, SR.I3D_SEED
SAMPLES = 2048
LEGS = (('', torch.float32, 8), ('f64_', torch.float64, 8), ('f32t4_', torch.float32, 4))


def sg_run(model, x, target, z, sigma, dtype):
    """x [1,C,T,H,W] in `dtype`, z [n,C,T,H,W] float64.  The semantics of DESIGN 15 with the moments in `dtype`."""
    G1, G2 = torch.zeros_like(x), torch.zeros_like(x)
    scores = []
    for k in range(len(z)):
        p = (x.double() + float(sigma) * torch.from_numpy(z[k])[None]).to(dtype).requires_grad_()
        s = model(p)[0, target]
        s.backward()
        G1 += p.grad
        G2 += p.grad * p.grad
        scores.append(float(s))
    n = float(len(z))
    G1, G2 = G1[0].double().numpy(), G2[0].double().numpy()      # [C,T,H,W]
    sg, sq = np.abs(G1 / n).sum(0), (G2 / n).sum(0)
    var = ((G2 - G1 * (G1 / n)) / (n - 1)).sum(0)
    with torch.no_grad():
        score_x = float(model(x)[0, target])
    return dict(sg=sg, sq=sq, var=var, sg_frames=sg.sum((1, 2)), sq_frames=sq.sum((1, 2)), var_frames=var.sum((1, 2)),
                sample_scores=np.array(scores), score_x=score_x, g2_total=G2.sum(),
                cancellation=SR.cancellation(var, G2, len(z)))


def gen_smoothgrad():
    out = {'n': np.array(N), 'level': np.array(LEVEL), 'seed': np.array(SEED), 'clips': np.array(CLIPS)}
    for leg, dtype, threads in LEGS:
        torch.set_num_threads(threads)
        torch.set_default_dtype(dtype)
        try:
            m = MG._i3d(False).to(dtype)
            for p in m.parameters():
                p.requires_grad_(False)
            for cid in CLIPS:
                x32 = R.clip(cid)[None]
                C, T, H, W = x32.shape[1:]
                z = SR.noise(SEED, range(N), C, T, H * W).reshape(N, C, T, H, W)
                sigma = SR.sigma_ref(x32, LEVEL)[0]
                x = torch.from_numpy(x32).to(dtype)
                if leg == '':
                    with torch.no_grad():
                        out[f'c{cid}_target'] = np.array(int(torch.argmax(m(x)[0])))
                    out[f'c{cid}_sigma'] = np.array(sigma, dtype=np.float32)
                target = int(out[f'c{cid}_target'])
                r = sg_run(m, x, target, z, sigma, dtype)
                tag = f'{leg}c{cid}'
                idx = MG.sample_idx(f'g/smoothgrad/{cid}', r['sg'].size, SAMPLES)
                if leg == '':
                    out[f'{tag}_idx'] = idx
                for key in ('sg', 'sq', 'var'):
                    out[f'{tag}_{key}_val'] = r[key].ravel()[idx]
                for key in ('sg_frames', 'sq_frames', 'var_frames', 'sample_scores', 'score_x', 'g2_total', 'cancellation'):
                    out[f'{tag}_{key}'] = np.asarray(r[key], dtype=np.float64)
                print(tag, 'sigma', sigma, 'sum sg', r['sg'].sum(), 'sum sq', r['sq'].sum(), 'sum var', r['var'].sum(),
                      'cancellation', r['cancellation'], flush=True)
                MG.save('smoothgrad', **out)
        finally:
            torch.set_default_dtype(torch.float32)
            torch.set_num_threads(8)


if __name__ == '__main__':
    gen_smoothgrad()
