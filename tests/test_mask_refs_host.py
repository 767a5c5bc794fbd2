"""CPU test of tests/mask_refs.py: the fp64 references and the derived gates that test_gpu_mask_kernels.py holds the
freeze and blob-staging kernels to are sound on the very inputs those tests run, before any kernel is compared.

* a numpy float32 restatement of each kernel's arithmetic (unfused, the backward summed in the kernel's own order:
  per-thread chain over the trips, 64-lane shuffle tree, four waves, 64 block partials in sequence) stays inside the
  gates on every case;
* wrong kernels land outside: in the forward, m[u-1] for m[u] and a `prev` that is not carried, each >= 100x; in the
  backward, m[u] for m[u+1] in the scan, P[u] for P[u-1], a dropped last trip, a block partial left out of the
  reduction, and swapped channel lanes.  The factors are recorded (conftest.note).  The sum bound grows with n = C*HW,
  so a dropped 1/64 of a 37635-term sum is only a few times the gate and a single dropped pixel is inside it: the
  exact cases close that hole, and this file proves that they are exact;
* the blob-staging reference equals a plain gather by the kernels' source-frame rule.
"""
import numpy as np
import pytest
import torch

import mask_refs as M
from conftest import note

F32 = np.float32
RUNS = M.freeze_runs()
RUN_IDS = [f"{n}-{'perclip' if pc else 'shared'}" for n, pc in RUNS]


def _fwd(x, rows, dtype, m_shift=0, carry=True):
    """P in `dtype`, the kernels' expression (1 - m) * x + m * prev with every operation rounded (no FMA); m_shift 1
    and carry False are the mutants"""
    x, m = x.numpy().astype(dtype), rows.numpy().astype(dtype)
    B, C, T, HW = x.shape
    P = np.empty_like(x)
    P[:, :, 0] = x[:, :, 0]
    for u in range(1, T):
        mu = m[:, u - m_shift].reshape(B, 1, 1)
        prev = P[:, :, u - 1] if carry else x[:, :, u - 1]
        P[:, :, u] = ((dtype(1) - mu) * x[:, :, u]).astype(dtype) + (mu * prev).astype(dtype)
    return P


def _scan(g, rows, dtype, m_shift=1):
    """G[u] = g[u] + m[u + m_shift] G[u+1] in `dtype` (m_shift 0 is the mutant)"""
    g, m = g.numpy().astype(dtype), rows.numpy().astype(dtype)
    B, C, T, HW = g.shape
    G = np.empty_like(g)
    G[:, :, T - 1] = g[:, :, T - 1]
    for u in range(T - 2, -1, -1):
        G[:, :, u] = g[:, :, u] + (m[:, u + m_shift].reshape(B, 1, 1) * G[:, :, u + 1]).astype(dtype)
    return G


def _terms(P, x, G):
    """[B,T,C*HW] terms (P[u-1] - X[u]) G[u] in the dtype of the operands, flat index i = c * HW + px; row u = 0 is 0"""
    B, C, T, HW = x.shape
    t = np.zeros_like(P)
    t[:, :, 1:] = ((P[:, :, :-1] - x[:, :, 1:]).astype(P.dtype) * G[:, :, 1:]).astype(P.dtype)
    return np.ascontiguousarray(t.transpose(0, 2, 1, 3)).reshape(B, T, C * HW)


def _kernel_order_sum32(t, inner):
    """fp32 sum of t [B,T,items*inner] the way freeze_bwd / freeze_bwd_cl4 + freeze_bwd_reduce do it: thread j of the
    16384 of a clip chains items j, j + 16384, ... (each item `inner` terms long, in order), lane 0 of each wave
    collects its 64 lanes by the shfl_down tree, the block adds its four waves in order, and the reduce kernel adds
    the 64 block partials in order.  Blocks that hold no item contribute +0.0 and are left out."""
    B, T, n = t.shape
    items = n // inner
    threads = min(-(-items // 256) * 256, M.BWD_THREADS)
    trips = -(-items // threads)
    pad = np.zeros((B, T, trips * threads, inner), F32)
    pad[:, :, :items] = t.reshape(B, T, items, inner)
    pad = pad.reshape(B, T, trips, threads, inner)
    acc = np.zeros((B, T, threads), F32)
    for k in range(trips):
        for c in range(inner):
            acc = (acc + pad[:, :, k, :, c]).astype(F32)
    v = acc.reshape(B, T, threads // 256, 4, 64)
    o = 32
    while o > 0:
        v = (v[..., :o] + v[..., o:2 * o]).astype(F32)
        o >>= 1
    v = v[..., 0]
    blk = (((v[..., 0] + v[..., 1]).astype(F32) + v[..., 2]).astype(F32) + v[..., 3]).astype(F32)
    s = np.zeros((B, T), F32)
    for k in range(blk.shape[2]):
        s = (s + blk[:, :, k]).astype(F32)
    return s


def _factor(mut, ref, bound):
    """how far a mutant's dmask lies from the reference, in units of the gate, over the entries (b, u >= 1) whose gate
    is not zero: (largest, median)"""
    r = (np.abs(mut - ref)[:, 1:] / np.where(bound[:, 1:] > 0, bound[:, 1:], np.inf)).reshape(-1)
    return float(r.max()), float(np.median(r))


def test_case_table_reaches_every_dispatch_path():
    seen = set()
    for name, (B, C, T, HW) in M.FREEZE_CASES.items():
        for cpad in M.out_layouts(C):
            for dx in (False, True):
                seen.add(M.bwd_kernel(C, T, cpad, dx))
    assert seen == {('generic', 16), ('generic', 32), ('generic', 64), ('cl4', 16), ('cl4', 32)}
    B, C, T, HW = M.FREEZE_CASES['F1']
    assert -(-C * HW // M.BWD_THREADS) == 3 and (C * HW) % 256 != 0
    B, C, T, HW = M.FREEZE_CASES['F2']
    assert -(-HW // M.BWD_THREADS) == 2 and -(-C * HW // M.BWD_THREADS) == 4 and M.bwd_kernel(C, T, 4, False) == ('cl4', 16)
    assert M.bwd_kernel(4, 40, 4, False) == ('generic', 64) and M.bwd_kernel(3, 16, 4, True) == ('generic', 16)
    B, C, T, HW = M.FREEZE_CASES['F9']
    cap = 2048 * 256
    assert -(-B * C * HW // cap) == 4 and -(-B * HW // cap) == 2 and B * C * T * HW * 4 < 14e6
    assert max(s[0] for s in M.FREEZE_CASES.values()) > 64 and any(s[1] > 4 for s in M.FREEZE_CASES.values())
    assert {s[2] for s in M.FREEZE_CASES.values()} >= {1, 17, 64}
    for B, T in ((130, 40), (7, 32)):
        m = M.freeze_masks(B, T)
        assert float(m.min()) >= 0 and float(m.max()) <= 1
        assert bool((m[2] == 0).all()) and bool((m[3] == 1).all())
        assert bool((m[1] == 0).any()) and bool((m[1] == 1).any()) and bool(((m[1] > 0) & (m[1] < 1)).any())
        assert set(m[4].tolist()) <= set(torch.sigmoid(torch.tensor([-5.0, 5.0])).tolist())


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_freeze_forward_gate(run):
    name, per_clip = run
    B, C, T, HW = M.FREEZE_CASES[name]
    c = M.freeze_case(name, per_clip)
    x, rows = c['x'], c['rows'].contiguous()
    assert float(x.min()) >= 0 and float(x.max()) <= 255
    P, bP = c['P'].numpy(), c['bP'].numpy()
    assert float(np.abs(M.freeze_fwd_ref(x, rows).numpy() - P).max()) == 0.0
    P32 = _fwd(x, rows, F32)
    assert np.array_equal(P32[:, :, 0], x.numpy()[:, :, 0]) and bool((bP[:, :, 0] == 0).all())
    err = np.abs(P32.astype(np.float64) - P)
    assert bool((err <= bP).all()), f"fp32 restatement leaves the gate by {float((err - bP).max()):.3e}"
    worst = float((err[:, :, 1:] / bP[:, :, 1:]).max()) if T > 1 else 0.0
    msg = f"mask host {name} per_clip={per_clip} fwd: fp32 restatement worst err/gate {worst:.3f}"
    if T > 1:
        # mutants (fp64, so that what is measured is the mutation and not rounding)
        f_m = float((np.abs(_fwd(x, rows, np.float64, m_shift=1) - P)[:, :, 1:] / bP[:, :, 1:]).max())
        assert f_m >= 100, f"m[u-1] for m[u] moves P by only {f_m:.1f}x the gate"
        msg += f"; m[u-1] for m[u] {f_m:.3g}x"
    if T > 2:       # (with T = 2 the only step reads P[0] = X[0]: nothing is carried)
        f_c = float((np.abs(_fwd(x, rows, np.float64, carry=False) - P)[:, :, 1:] / bP[:, :, 1:]).max())
        assert f_c >= 100, f"a prev that is not carried moves P by only {f_c:.1f}x the gate"
        msg += f"; prev not carried {f_c:.3g}x"
    note(msg)


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_freeze_backward_gate(run):
    name, per_clip = run
    B, C, T, HW = M.FREEZE_CASES[name]
    n = C * HW
    c = M.freeze_case(name, per_clip)
    x, g, rows = c['x'], c['g'], c['rows'].contiguous()
    ref, bound, sabs = c['dmask'].numpy(), c['b_dmask'].numpy(), c['sabs'].numpy()
    # the reference: autograd == the explicit formula; entry 0 is exactly 0; the terms do not cancel
    assert float(np.abs(ref - c['formula'].numpy()).max()) <= 1e-11 * (float(sabs.max()) + 1e-300)
    assert bool((ref[:, 0] == 0).all()) and bool((bound[:, 0] == 0).all())
    if T == 1:
        assert bool((ref == 0).all()) and torch.equal(c['dx'], g.double())
        return
    assert bool((np.abs(ref[:, 1:]) >= 0.1 * sabs[:, 1:]).all()), "terms of some dmask entry cancel"
    assert bool((sabs[:, 1:] > 0).all())
    # fp32 restatement in the order of both kernels
    P32, G32 = _fwd(x, rows, F32), _scan(g, rows, F32)
    t32 = _terms(P32, x.numpy(), G32)
    got = {'generic': _kernel_order_sum32(t32, 1)}
    if C <= 4 and T <= 32:      # one thread per pixel, its channels in sequence
        got['cl4'] = _kernel_order_sum32(np.ascontiguousarray(t32.reshape(B, T, C, HW).transpose(0, 1, 3, 2)).reshape(B, T, n), C)
    msg = f"mask host {name} per_clip={per_clip} bwd:"
    for k, v in got.items():
        err = np.abs(v.astype(np.float64) - ref)
        assert bool((err <= bound).all()), f"{k}: fp32 restatement leaves the dmask gate by {float((err - bound).max()):.3e}"
        assert bool((v[:, 0] == 0).all())
        msg += f" {k} restatement err/gate {float((err[:, 1:] / bound[:, 1:]).max()):.4f}"
    m32 = rows.numpy().astype(F32)
    dx32 = G32.copy()
    dx32[:, :, 1:] = ((F32(1) - m32[:, 1:]).reshape(B, 1, T - 1, 1) * G32[:, :, 1:]).astype(F32)
    err = np.abs(dx32.astype(np.float64) - c['dx'].numpy())
    assert bool((err <= c['b_dx'].numpy()).all())
    nz = c['b_dx'].numpy() > 0
    msg += f" dx err/gate {float((err[nz] / c['b_dx'].numpy()[nz]).max()):.3f}"
    # mutants, fp64
    xd, P, G = x.double().numpy(), c['P'].numpy(), c['G'].numpy()
    t64 = _terms(P, xd, G)
    assert float(np.abs(t64.sum(-1) - ref).max()) <= 1e-11 * float(sabs.max())
    fac = {}
    Gm = _scan(g, rows, np.float64, m_shift=0)
    if T > 2:
        fac['m[u] for m[u+1]'] = _factor(_terms(P, xd, Gm).sum(-1), ref, bound)
    else:       # T = 2: the scan's only step feeds G[0], which no dmask entry reads; dx[0] = G[0] shows it
        f_dx = float((np.abs(Gm[:, :, 0] - c['dx'].numpy()[:, :, 0]) / c['b_dx'].numpy()[:, :, 0]).max())
        fac['m[u] for m[u+1] (on dx[0])'] = (f_dx, f_dx)
    Pshift = np.concatenate([P[:, :, 1:], P[:, :, -1:]], axis=2)          # P[u] where P[u-1] belongs
    fac['P[u] for P[u-1]'] = _factor(_terms(Pshift, xd, G).sum(-1), ref, bound)
    # A dropped share f of n like-signed terms moves the sum by f, and the sum bound is 2 (n-1) 2^-24 of it: such a
    # mutant must leave the gate where f / (2 (n-1) 2^-24) is well above 1 (asserted from 4 on, the margin for terms of
    # unequal size) and cannot where it is below (F9: 1/64 of 150528 terms is 0.87 gates).  The exact cases, F9's shape among them, hold those.
    must = {}

    def dropped(key, kept):
        fac[key] = _factor(kept.sum(-1), ref, bound)
        must[key] = (1.0 - kept.shape[-1] / n) / (2 * (n - 1) * M.U) >= 4

    if n > M.BWD_THREADS:
        dropped('last trip dropped', t64[:, :, :(n - 1) // M.BWD_THREADS * M.BWD_THREADS])
    if 'cl4' in got and HW > M.BWD_THREADS:
        last = (HW - 1) // M.BWD_THREADS * M.BWD_THREADS
        dropped('last trip dropped (cl4)', np.ascontiguousarray(t64.reshape(B, T, C, HW)[..., :last]).reshape(B, T, C * last))
    blk = min(63, (n - 1) // 256)               # the last block that holds anything
    dropped(f'block {blk} left out', t64[:, :, (np.arange(n) // 256) % 64 != blk])
    if C > 1:
        perm = [ch ^ 1 if (ch ^ 1) < C else ch for ch in range(C)]
        fac['lanes c, c+1 swapped'] = _factor(_terms(P, xd, _scan(g[:, perm], rows, np.float64)).sum(-1), ref, bound)
    for k, (mx, med) in fac.items():
        if must.get(k, True):
            assert mx > 1, f"{name}: mutant '{k}' stays inside the gate ({mx:.2f}x)"
        msg += f"; {k} {mx:.3g}x (median {med:.3g}x)" + ("" if must.get(k, True) else " [share too small for the sum bound at this n]")
    note(msg)
    # Below 10x (recorded above): a dropped block or last trip of the long sums, and swapped lanes at F2 / F9 (the
    # sum bound is 0.7 % to 1.8 % of the sum there).  The exact cases hold those to bit equality with the same kernels;
    # a swap of lane 2 with the pad lane of a 3-channel row reads a NaN.  The two index slips must stay well outside.
    for k, (mx, _) in fac.items():
        if k.startswith(('m[u]', 'P[u]')):
            assert mx >= 10, f"{name}: mutant '{k}' is only {mx:.1f}x outside the gate"


@pytest.mark.parametrize("run", M.exact_runs(), ids=lambda r: f"{r[0]}-{'perclip' if r[1] else 'shared'}")
def test_exact_cases_are_exact(run):
    """Every intermediate of the float64 run is a float32 number, and sum|term| of every dmask entry is below 2^24
    units of the terms' last place (1/16): every fp32 partial sum, in any order, is then exact, and the kernel must
    reproduce the float64 result bit for bit.  Every probe element matters: leaving it out changes dmask."""
    name, per_clip = run
    B, C, T, HW = M.FREEZE_CASES[name]
    c = M.exact_case(name, per_clip)
    x, g, rows = c['x'], c['g'], c['rows']
    assert torch.equal(x, x.round()) and float(x.min()) >= 0 and float(x.max()) <= 255
    assert set(c['masks'].unique().tolist()) <= {0.0, 0.5, 1.0} and int((c['masks'] == 0.5).sum(1).max()) <= 2
    assert torch.equal(g, g.round()) and float(g.abs().max()) <= 3
    n = C * HW
    for b in (0, B - 1):
        idx = c['probes'][b]
        assert len(idx) <= 64
        must = [0, 255, 256, 16383, 16384, 16385, n - 1, HW - 1, HW] + \
               [k * M.BWD_THREADS - d for k in range(1, n // M.BWD_THREADS + 1) for d in (1, 0)]
        assert all(i in idx for i in must if 0 <= i < n)
        flat = g[b].permute(0, 2, 1).reshape(n, T)
        assert sorted(torch.nonzero(flat.abs().sum(1)).view(-1).tolist()) == idx
    xd = x.double().numpy()
    P, G = c['P'].numpy(), c['G'].numpy()
    t64 = _terms(P, xd, G)
    for v in (P, G, t64, c['dx'].numpy(), c['dmask'].numpy(), P[:, :, :-1] - xd[:, :, 1:]):
        assert np.array_equal(v.astype(F32).astype(np.float64), v)
        assert np.array_equal(np.round(v * 16), v * 16)
    assert float(c['sabs'].max()) * 16 < 2 ** 24
    assert np.array_equal(t64.sum(-1), c['dmask'].numpy())
    # the fp32 restatement, in kernel order, is the float64 result
    t32 = _terms(_fwd(x, rows.contiguous(), F32), x.numpy(), _scan(g, rows.contiguous(), F32))
    assert np.array_equal(_kernel_order_sum32(t32, 1).astype(np.float64), c['dmask'].numpy())
    # every probe of the first and last clip changes some dmask entry when it is left out
    for b in (0, B - 1):
        assert bool((np.abs(t64[b][:, c['probes'][b]]).sum(0) > 0).all())
    note(f"mask host exact {name} per_clip={per_clip}: max sum|term| {float(c['sabs'].max()):.0f} (limit {2 ** 20}), "
         f"probes per clip {min(map(len, c['probes']))}..{max(map(len, c['probes']))}, nonzero dmask entries "
         f"{int((c['dmask'] != 0).sum())} of {B * (T - 1)}")
    assert int((c['dmask'] != 0).sum()) >= B * (T - 1) // 2


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(M.BLOB_CASES))
def test_blob_reference_is_a_gather(name, mode):
    import ivf_lib as L
    b, C, T, HW, ml = M.BLOB_CASES[name]
    tab = M.blob_table(T, ml).numpy()
    n = tab.shape[0]
    assert n == L.lib().ivf_blob_count(T, ml)
    assert [tuple(r) for r in tab] == [(a, ln) for ln in range(1, ml + 1) for a in range(T - ln + 1)]
    x = M.blob_input(name).numpy()
    ref = M.blob_ref(name, mode).numpy().reshape(b, n, C, T, HW)
    for k, (a, ln) in enumerate(tab):
        src = [M.blob_src(u, int(a), int(ln), mode) for u in range(T)]
        assert np.array_equal(ref[:, k].view(np.int32), x[:, :, src].view(np.int32))
    first, count = M.blob_chunks(b, n)[1]
    assert 0 < first < n < first + count < 2 * n


def test_blob_table_covers_the_listed_shapes():
    cs = M.BLOB_CASES.values()
    assert {c[1] for c in cs} >= {1, 3, 4} and {c[2] for c in cs} >= {2, 9, 16, 64}
    assert any(c[4] < c[2] for c in cs) and {c[3] % 4 for c in cs} >= {0, 3}
    b, C, T, HW, ml = M.BLOB_CASES['S5']
    rows = b * 3
    assert rows * HW > 2048 * 256 and rows * C * HW // 4 > 2048 * 256 and rows * T * HW * 4 * 4 <= 20e6
