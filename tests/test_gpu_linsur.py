"""KernelSHAP and LIME (csrc/linsur_ops.hip) on the GPU: the sampled rows against the numpy rows, the
staging kernel against ivf_stmask_expand_fwd + ivf_stfreeze_fwd on each row's explicit per-frame S (equality), the
fp64 moments against the reference loops (equality), the Cholesky solve against the accurate fp64 solution at the gate
of tests/linsur_refs.py, the singular and regular sampled systems, the score rows on the plans against
st_perturbed_forward and against tests/golden/linsur.npz (make_golden_linsur.py: the reference's I3D model under the
torch restatement of expand and per-pixel freeze), and the public surfaces.  tests/test_linsur_refs_host.py proves the
references on the CPU."""
import functools
import pickle

import numpy as np
import pytest
import torch

import box_refs as B
import linsur_refs as LR
import rise_refs as RR
import shap_refs as SH
import stmask_refs as SR
from conftest import note, rel_err_elem
from test_gpu_box import FLOOR, _gate
from test_gpu_leaf_kernels import bits, guarded, untouched
from test_gpu_shapley import _kth_clstm, _s16_x, _tg, clstm, s16, smth_model      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00ABC
SEED = 1234


def _dev_bits(Z):
    """numpy rows as the int32 device tensor the entries take (the uint32 words)"""
    return torch.from_numpy(LR.pack(Z).view(np.int32)).cuda().contiguous()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _table(P):
    return torch.from_numpy(np.concatenate([LR.size_table(P), np.zeros(1, np.uint32)]).view(np.int32)).cuda()


# ---------------------------------------------------------------------------------------------------- A. rows
@pytest.mark.parametrize("paired", [1, 0])
@pytest.mark.parametrize("grid,first_k,count", [((1, 1, 2), 0, 6), ((1, 3, 11), 0, 6), ((3, 3, 4), 0, 6), ((3, 3, 4), 3, 5),
                                                ((4, 16, 16), 0, 4), ((4, 16, 16), 1001, 3)])
def test_kshap_rows_are_the_numpy_rows(grid, first_k, count, paired):
    import ivf_lib as L
    P = grid[0] * grid[1] * grid[2]
    nw = (P + 31) // 32
    bb, bt = guarded((count, nw), dtype=torch.int32, sent=-77)
    bs, sz = guarded((count,), dtype=torch.int16, sent=-77)
    bt.fill_(0x5ABCDEF0)
    sz.fill_(0x7ABC)
    L.check(L.lib().ivf_kshap_rows(SEED, paired, first_k, count, *grid, L.ptr(_table(P)), L.ptr(bt), L.ptr(sz), L.stream()))
    torch.cuda.synchronize()
    assert untouched(bb, -77) and untouched(bs, -77)
    Z, s = LR.kshap_rows(SEED, count, P, bool(paired), first_k)
    got = _u32(bt)
    assert np.array_equal(got, LR.pack(Z)), (grid, first_k, count, paired)
    assert np.array_equal(sz.cpu().numpy().astype(np.int64), s)
    if P % 32:
        assert not (got[:, -1] >> np.uint32(P % 32)).any(), "unused high bits are not zero"
    assert np.array_equal(LR.unpack(got, P).sum(axis=1), s) and s.min() >= 1 and s.max() <= P - 1
    if paired and first_k % 2 == 0:
        assert np.array_equal(LR.unpack(got, P)[1::2], ~LR.unpack(got, P)[0:2 * (count // 2):2])


@pytest.mark.parametrize("grid,first_k,count", [((1, 1, 2), 0, 6), ((1, 3, 11), 2, 6), ((3, 3, 4), 0, 6), ((4, 16, 16), 7, 3)])
def test_lime_rows_are_the_rise_masks(grid, first_k, count):
    import ivf_lib as L
    P = grid[0] * grid[1] * grid[2]
    nw = (P + 31) // 32
    th = RR.thresh(0.37)
    bb, bt = guarded((count, nw), dtype=torch.int32, sent=-77)
    bt.fill_(0x5ABCDEF0)
    S = torch.empty((count,) + grid, device='cuda')
    L.check(L.lib().ivf_lime_rows(SEED, th, first_k, count, *grid, L.ptr(bt), L.stream()))
    L.check(L.lib().ivf_rise_masks(SEED, th, first_k, count, *grid, L.ptr(S), L.stream()))
    torch.cuda.synchronize()
    assert untouched(bb, -77)
    got = _u32(bt)
    assert np.array_equal(LR.unpack(got, P), S.cpu().numpy().reshape(count, P) == 1.0)
    assert np.array_equal(got, LR.pack(LR.lime_rows(SEED, th, count, P, first_k)))
    if P % 32:
        assert not (got[:, -1] >> np.uint32(P % 32)).any(), "unused high bits are not zero"
    assert 0 < LR.unpack(got, P).sum() < count * P


def test_rows_known_answer_on_the_device():
    import ivf_lib as L
    bt = torch.empty(4, 1, dtype=torch.int32, device='cuda')
    sz = torch.empty(4, dtype=torch.int16, device='cuda')
    L.check(L.lib().ivf_kshap_rows(1234, 1, 0, 4, 2, 2, 2, L.ptr(_table(8)), L.ptr(bt), L.ptr(sz), L.stream()))
    assert _u32(bt).tolist() == [[2], [253], [223], [32]] and sz.cpu().tolist() == [1, 7, 7, 1]
    L.check(L.lib().ivf_kshap_rows(1234, 0, 0, 4, 2, 2, 2, L.ptr(_table(8)), L.ptr(bt), L.ptr(sz), L.stream()))
    assert _u32(bt).tolist() == [[2], [254], [223], [29]] and sz.cpu().tolist() == [1, 7, 7, 4]
    b2 = torch.empty(2, 2, dtype=torch.int32, device='cuda')
    L.check(L.lib().ivf_kshap_rows(1234, 1, 0, 2, 3, 3, 4, L.ptr(_table(36)), L.ptr(b2), L.ptr(sz), L.stream()))
    assert _u32(b2).tolist() == [[4751616, 0], [4290215679, 15]] and sz.cpu().tolist()[:2] == [4, 32]
    L.check(L.lib().ivf_lime_rows(1234, 1 << 31, 0, 2, 3, 3, 4, L.ptr(b2), L.stream()))
    assert _u32(b2).tolist() == [[1761322299, 1], [26859718, 2]]
    assert LR.size_table(8).tolist() == [946549266, 1498703005, 1940425995, 2354541300, 2796264290, 3348418029]


# ---------------------------------------------------------------------------------------------------- B. staging
def _stage(xd, AHd, AWd, dims, bd, first, count, cpad):
    import ivf_lib as L
    b, C, T, H, W, (gt, gh, gw), n = dims
    buf, out = guarded((count, C, T, H * W) if cpad == 0 else (count, T, H * W, 4))
    bits(out).fill_(NAN_BITS)
    L.check(L.lib().ivf_lin_stage(L.ptr(xd), b, C, T, H, W, L.ptr(AHd), L.ptr(AWd), gt, gh, gw, n, L.ptr(bd), first, count,
                                  L.ptr(out), cpad, L.stream()))
    torch.cuda.synchronize()
    assert untouched(buf), f"lin_stage out_cpad={cpad}: a sentinel row was written"
    assert not bool(torch.isnan(out).any()), f"lin_stage out_cpad={cpad}: an element was never written"
    return out


def _pair(xd, AHd, AWd, dims, Z, first, count, cpad):
    """the same rows by ivf_stmask_expand_fwd + ivf_stfreeze_fwd on the explicit per-frame S of each row"""
    import ivf_lib as L
    b, C, T, H, W, grid, n = dims
    gt, gh, gw = grid
    rows = np.arange(first, first + count)
    S = torch.from_numpy(RR.frame_masks(LR.row_masks(Z, grid, rows % (n + 1)), T)).cuda().contiguous()   # [count,T,gh,gw]
    xr = xd[torch.from_numpy(rows // (n + 1)).cuda()].contiguous()
    M = torch.empty(count, T, H, W, device='cuda')
    L.check(L.lib().ivf_stmask_expand_fwd(L.ptr(S), L.ptr(AHd), L.ptr(AWd), L.ptr(M), count, T, gh, gw, H, W, L.stream()))
    out = torch.empty((count, C, T, H * W) if cpad == 0 else (count, T, H * W, 4), device='cuda')
    L.check(L.lib().ivf_stfreeze_fwd(L.ptr(xr), L.ptr(M), L.ptr(out), count, C, T, H * W, cpad, L.stream()))
    torch.cuda.synchronize()
    return out


def _check_windows(C, T, sigma, grid, cpad, windows, H=12, W=20, b=2, n=4, seed=SEED, kind="kshap"):
    gt, gh, gw = grid
    P = gt * gh * gw
    per = n + 1
    dims = (b, C, T, H, W, grid, n)
    xd = B.stage_inputs(b, C, T, H, W, key='shap').cuda()
    AHd, AWd = SR.axis_weights(H, gh, sigma).cuda(), SR.axis_weights(W, gw, sigma).cuda()
    Z = LR.kshap_rows(seed, n, P)[0] if kind == "kshap" else LR.lime_rows(seed, RR.thresh(0.5), n, P)
    bd = _dev_bits(Z)
    moved = 0
    for first, count in windows:
        assert 0 <= first and first + count <= b * per
        got = _stage(xd, AHd, AWd, dims, bd, first, count, cpad)
        want = _pair(xd, AHd, AWd, dims, Z, first, count, cpad)
        assert torch.equal(got, want), f"rows [{first}, {first + count}) of {b * per}: not the bits of expand_fwd + stfreeze_fwd"
        if cpad == 4:
            assert torch.equal(bits(got[..., C:]), torch.zeros_like(bits(got[..., C:]))), "pad lane not +0.0"
        src = xd[torch.from_numpy(np.arange(first, first + count) // per).cuda()]
        flat = got if cpad == 0 else got[..., :C].permute(0, 3, 1, 2)
        moved += int((flat != src.reshape(count, C, T, H * W)).any(dim=(1, 2, 3)).sum())
    assert moved > 0, "no staged row differs from its clip: the comparison is vacuous"


# n = 4: 5 rows a clip, 10 in all.  Inside clip 0, across the clip boundary (row 5 = n + 1), ending on the last row, the
# whole list
WINDOWS = [(1, 3), (3, 4), (7, 3), (0, 10)]


@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("sigma", [0.0, 1.5])
@pytest.mark.parametrize("C", [1, 3])
def test_staging_is_expand_plus_freeze_on_the_explicit_mask(C, sigma, cpad):
    """B.  b = 2, T = 5, 12 x 20 (one workgroup with 16 idle threads), grid (3, 3, 4), n = 4"""
    _check_windows(C, 5, sigma, (3, 3, 4), cpad, WINDOWS)


@pytest.mark.parametrize("cpad", [0, 4])
def test_staging_over_several_workgroups(cpad):
    """23 x 27 = 621 pixels: three workgroups per row, the last ragged, rows of pixels that straddle workgroups, LIME
    rows of a second seed; then the widest grid row (32 cells: bit 31 of the column word) with 192 players, whose bit
    rows are six words long"""
    _check_windows(3, 6, 1.0, (2, 4, 5), cpad, [(2, 7), (0, 14)], H=23, W=27, n=6, seed=99, kind="lime")
    _check_windows(2, 3, 0.7, (3, 2, 32), cpad, [(3, 5), (0, 8)], H=9, W=40, n=3, seed=5)


@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("T", [16, 17])
def test_staging_on_both_frame_loop_paths(T, cpad):
    """T = 17 (the frame loop) and T = 16 (pieces of 16 preloaded frames), one temporal cell per frame"""
    _check_windows(3, T, 1.5, (T, 1, 2), cpad, [(1, 3), (3, 5)])


@pytest.mark.parametrize("cpad", [0, 4])
def test_row_n_is_the_fully_frozen_clip(cpad):
    """sigma 0, 12 x 16 on a (3, 4) grid: the bilinear weights are multiples of 1/8, exact in fp32, so the fully set
    mask expands to exactly 1 and row n is ivf_blob_stage's fully frozen row (the blob [0, T)), bit for bit"""
    import ivf_lib as L
    b, C, T, H, W, n, grid = 2, 3, 5, 12, 16, 4, (3, 3, 4)
    xd = B.stage_inputs(b, C, T, H, W, key='shap').cuda()
    AHd, AWd = SR.axis_weights(H, 3, 0.0).cuda(), SR.axis_weights(W, 4, 0.0).cuda()
    Z, _ = LR.kshap_rows(SEED, n, 36)
    got = _stage(xd, AHd, AWd, (b, C, T, H, W, grid, n), _dev_bits(Z), 0, b * (n + 1), cpad)
    nb = L.lib().ivf_blob_count(T, T)
    frozen = torch.empty((b,) + tuple(got.shape[1:]), device='cuda')
    for r in range(b):                                   # candidate nb - 1 of each clip: length T from frame 0
        L.check(L.lib().ivf_blob_stage(L.ptr(xd), b, C, T, H * W, T, 0, r * nb + nb - 1, 1, L.ptr(frozen[r]), cpad, L.stream()))
    torch.cuda.synchronize()
    for cl in range(b):
        assert torch.equal(bits(got[cl * (n + 1) + n]), bits(frozen[cl])), f"clip {cl}: row n is not the frozen clip"
        assert not torch.equal(bits(got[cl * (n + 1)]), bits(frozen[cl]))


# ---------------------------------------------------------------------------------------------------- C. moments
def _moments(Z, s, sx, wtab):
    import ivf_lib as L
    n, P = Z.shape
    b = s.shape[0]
    f64 = dict(dtype=torch.float64, device='cuda')
    bN, N = guarded((P, P), dtype=torch.float64)
    br, r = guarded((b, P), dtype=torch.float64)
    v, Wsum, t, wrow = torch.full((P,), np.nan, **f64), torch.full((1,), np.nan, **f64), torch.full((b,), np.nan, **f64), \
        torch.full((n,), np.nan, **f64)
    N.fill_(float('nan'))
    r.fill_(float('nan'))
    ok = torch.full((b,), -77, dtype=torch.int32, device='cuda')
    wt = None if wtab is None else torch.from_numpy(np.asarray(wtab, np.float64)).cuda()
    L.check(L.lib().ivf_lin_moments(L.ptr(torch.from_numpy(s).cuda()), L.ptr(torch.from_numpy(sx).cuda()), L.ptr(_dev_bits(Z)),
                                    L.ptr(wt), b, n, P, L.ptr(N), L.ptr(v), L.ptr(Wsum), L.ptr(r), L.ptr(t), L.ptr(wrow),
                                    L.ptr(ok), L.stream()))
    torch.cuda.synchronize()
    assert untouched(bN) and untouched(br)
    return dict(N=N.cpu().numpy(), v=v.cpu().numpy(), Wsum=float(Wsum[0]), r=r.cpu().numpy(), t=t.cpu().numpy(),
                w=wrow.cpu().numpy(), ok=ok.cpu().numpy())


def _same_f64(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("P,n,weighted", [(36, 72, False), (36, 50, True), (33, 40, True), (2, 9, False), (1024, 48, False)])
def test_moments_are_the_reference_loops_bit_for_bit(P, n, weighted, b):
    g = np.random.default_rng(P + n + b)
    Z = LR.lime_rows(SEED, RR.thresh(0.5), n, P) if weighted else LR.kshap_rows(SEED, n, P)[0]
    s, sx = g.random((b, n + 1)).astype(np.float32), g.random(b).astype(np.float32)
    if b == 3:
        s[1, n // 2] = np.nan                                            # one clip with a NaN score
    wtab = LR.lime_wtab(P) if weighted else None
    got, want = _moments(Z, s, sx, wtab), LR.moments(Z, s, sx, wtab, exact_N=P == 1024)
    good = want["ok"].astype(bool)
    assert got["ok"].tolist() == want["ok"].tolist() == ([1] if b == 1 else [1, 0, 1])
    assert _same_f64(got["N"], want["N"]) and _same_f64(got["v"], want["v"]) and _same_f64(got["w"], want["w"])
    assert _same_f64(got["Wsum"], want["Wsum"])
    assert _same_f64(got["r"][good], want["r"][good]) and _same_f64(got["t"][good], want["t"][good])
    assert np.isfinite(got["r"][good]).all() and (weighted or float(got["N"].max()) == got["v"].max())
    if b == 3:                                                           # the other clips do not feel the NaN
        s2 = s.copy()
        s2[1, n // 2] = 0.5
        clean = _moments(Z, s2, sx, wtab)
        assert clean["ok"].tolist() == [1, 1, 1]
        assert _same_f64(clean["r"][[0, 2]], got["r"][[0, 2]]) and _same_f64(clean["t"][[0, 2]], got["t"][[0, 2]])
        # an infinite score_x is caught as well
        sx3 = sx.copy()
        sx3[2] = np.inf
        assert _moments(Z, s2, sx3, wtab)["ok"].tolist() == [1, 1, 0]


# ---------------------------------------------------------------------------------------------------- D. solve
def _solve(kind, mo, s, sx, P, ridge=0.0):
    """ivf_lin_solve on the REFERENCE's moments: (cells [b,P], intercept, total, ok)"""
    import ivf_lib as L
    lib = L.lib()
    b, n = s.shape[0], s.shape[1] - 1
    dev = [torch.from_numpy(np.ascontiguousarray(np.asarray(mo[k], np.float64).reshape(-1))).cuda() for k in ("N", "v", "Wsum", "r", "t")]
    ok = torch.from_numpy(np.asarray(mo["ok"], np.int32)).cuda()
    work = torch.empty(lib.ivf_lin_workspace_bytes(P), dtype=torch.uint8, device='cuda')
    bc, cells = guarded((b, P))
    bits(cells).fill_(NAN_BITS)
    icpt, total = torch.full((b,), -7.0, device='cuda'), torch.full((b,), -7.0, device='cuda')
    L.check(lib.ivf_lin_solve(kind, *[L.ptr(d) for d in dev], L.ptr(torch.from_numpy(s).cuda()), L.ptr(torch.from_numpy(sx).cuda()),
                              b, n, P, float(ridge), L.ptr(work), L.ptr(cells), L.ptr(icpt), L.ptr(total), L.ptr(ok), L.stream()))
    torch.cuda.synchronize()
    assert untouched(bc)
    return cells.cpu().numpy(), icpt.cpu().numpy(), total.cpu().numpy(), ok.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _solve_case(kind, m):
    """a sampled system with m unknowns and 3 right-hand sides, and its fp64 fit"""
    g = np.random.default_rng(100 * kind + m)
    if kind == 0:
        P = m + 1
        n = 4 * P
        Z, _ = LR.kshap_rows(SEED, n, P)
    else:
        P = m
        n = max(8, min(4 * P, 256))
        Z = LR.lime_rows(SEED, RR.thresh(0.5), n, P)
    s, sx = g.random((3, n + 1)).astype(np.float32), g.random(3).astype(np.float32)
    fit = LR.kshap_fit(Z, s, sx) if kind == 0 else LR.lime_fit(Z, s, sx, LR.lime_wtab(P), 1.0)
    return P, Z, s, sx, fit


@pytest.mark.parametrize("m", [1, 2, 31, 32, 33, 64, 65, 1023])
@pytest.mark.parametrize("kind", [0, 1])
def test_solve_meets_the_gate_at_every_block_edge(kind, m):
    """|phi_dev - phi*| <= 2^-24 |phi*| + 8 e_ref, e_ref the fp64 error of numpy's own solve (linsur_refs)"""
    P, Z, s, sx, fit = _solve_case(kind, m)
    assert not fit["singular"] and fit["ok"].tolist() == [1, 1, 1]
    cells, icpt, total, ok = _solve(kind, fit, s, sx, P, 1.0)
    assert ok.tolist() == [1, 1, 1] and np.isfinite(cells).all()
    err = np.abs(cells.astype(np.float64) - fit["cells"])
    lim = LR.gate(fit["cells"], fit["e_ref"])
    worst = float((err / lim).max())
    note(f"linsur solve kind {kind} m {m}: e_ref {fit['e_ref']:.2e}, worst err / gate {worst:.3f}")
    assert bool((err <= lim).all()), (kind, m, worst)
    assert np.array_equal(total, fit["total"].astype(np.float32))
    if kind == 0:
        assert not icpt.any()
        gap = np.abs(cells.astype(np.float64).sum(axis=1) - fit["total"])
        assert bool((gap <= P * 2.0 ** -24 * np.abs(cells.astype(np.float64)).sum(axis=1)).all()), gap     # efficiency
    else:
        e0 = np.abs(icpt.astype(np.float64) - fit["intercept"])
        assert bool((e0 <= _icpt_gate(fit)).all()), (e0, _icpt_gate(fit))


def _icpt_gate(fit):
    """intercept = t / Wsum - sum_c mu_c phi_c: the one fp32 rounding of the output, the cells' gated fp64 error carried
    through mu, and the P roundings of the fp64 dot product itself (2^-53 each, against the magnitudes summed)"""
    P = len(fit["mu"])
    dot = (np.abs(fit["mu"])[None, :] * np.abs(fit["cells"])).sum(axis=1) + np.abs(fit["t"] / fit["Wsum"])
    return 2.0 ** -24 * np.abs(fit["intercept"]) + 8.0 * fit["e_ref"] * np.abs(fit["mu"]).sum() + (P + 2) * 2.0 ** -53 * dot


@pytest.mark.parametrize("P,n,singular", [(8, 16, True), (1024, 2048, True), (16, 64, False), (392, 1568, False),
                                          (1024, 4096, False)])
def test_the_sampled_systems_come_out_as_the_pivot_rule_says(P, n, singular):
    """the paired systems of seed 1234: a singular one gives ok = 0 and NaN cells for EVERY clip, a regular one ok = 1"""
    g = np.random.default_rng(P)
    Z, _ = LR.kshap_rows(SEED, n, P)
    s, sx = g.random((2, n + 1)).astype(np.float32), g.random(2).astype(np.float32)
    mo = LR.moments(Z, s, sx, None, exact_N=True)
    cells, icpt, total, ok = _solve(0, mo, s, sx, P)
    if singular:
        assert ok.tolist() == [0, 0] and np.isnan(cells).all() and np.isnan(icpt).all()
    else:
        assert ok.tolist() == [1, 1] and np.isfinite(cells).all()
    assert np.array_equal(total, LR.totals(s, sx).astype(np.float32))


def test_a_clip_that_is_not_ok_gets_nan_and_leaves_the_others():
    P, Z, s, sx, fit = _solve_case(0, 32)
    mo = dict(fit, ok=np.array([1, 0, 1], np.int32))
    cells, icpt, total, ok = _solve(0, mo, s, sx, P)
    full = _solve(0, fit, s, sx, P)[0]
    assert ok.tolist() == [1, 0, 1] and np.isnan(cells[1]).all() and np.isnan(icpt[1])
    assert np.array_equal(cells[[0, 2]].view(np.uint32), full[[0, 2]].view(np.uint32))


def test_fit_quality_is_the_reference_chain():
    import ivf_lib as L
    for kind in (0, 1):
        P, Z, s, sx, fit = _solve_case(kind, 33)
        cells, icpt, total, ok = _solve(kind, fit, s, sx, P, 1.0)
        n = Z.shape[0]
        r2 = torch.full((3,), -7.0, device='cuda')
        dv = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt).reshape(-1))).cuda()    # noqa: E731
        okd = np.array([1, 1, 0], np.int32)
        L.check(L.lib().ivf_lin_fit(L.ptr(dv(s, np.float32)), L.ptr(dv(sx, np.float32)), L.ptr(_dev_bits(Z)),
                                    L.ptr(dv(fit["w"], np.float64)), L.ptr(dv(cells, np.float32)),
                                    L.ptr(dv(icpt, np.float32)) if kind else None, L.ptr(dv(fit["t"], np.float64)),
                                    L.ptr(dv([fit["Wsum"]], np.float64)), L.ptr(dv(okd, np.int32)), 3, n, P, L.ptr(r2),
                                    L.stream()))
        want = LR.r2_ref(Z, fit["w"], s, sx, cells, icpt, fit["t"], fit["Wsum"]).astype(np.float32)
        got = r2.cpu().numpy()
        assert np.array_equal(got[:2].view(np.uint32), want[:2].view(np.uint32)) and np.isnan(got[2]), (kind, got, want)
        assert bool((got[:2] < 1.0).all())


# ---------------------------------------------------------------------------------------------------- E. plans
def _chain(eng, x, targets, grid, sigma, n, math, kind):
    """lin_scores == st_perturbed_forward of the explicit expanded masks in the same chunk composition (equality); row
    n against Shapley's prefix-P score, which sits at another place of its chunk: the other-composition gate"""
    b, T = x.shape[0], x.shape[2]
    P = grid[0] * grid[1] * grid[2]
    per = n + 1
    Bp = eng.max_batch
    if kind == "kshap":
        bd, sizes = eng.kshap_rows(n, grid, SEED)
        Z, s = LR.kshap_rows(SEED, n, P)
        assert np.array_equal(sizes.cpu().numpy().astype(np.int64), s)
    else:
        bd = eng.lime_rows(n, 0.5, grid, SEED)
        Z = LR.lime_rows(SEED, RR.thresh(0.5), n, P)
    assert np.array_equal(_u32(bd), LR.pack(Z))
    scores = eng.lin_scores(x, targets, bd, grid, sigma)
    assert tuple(scores.shape) == (b, per)
    flat = scores.reshape(-1)
    tl = torch.as_tensor(targets, device='cuda').long()
    assert b * per > Bp and per % Bp != 0                 # several chunks, and they cross the clip boundary
    for first in range(0, b * per, Bp):
        rows = np.arange(first, min(first + Bp, b * per))
        S = torch.from_numpy(RR.frame_masks(LR.row_masks(Z, grid, rows % per), T)).cuda().contiguous()
        clip = torch.from_numpy(rows // per).cuda()
        M = eng.st_expand(S, grid[1:], sigma)
        pr = eng.st_perturbed_forward(x[clip].contiguous(), M)[torch.arange(len(rows), device='cuda'), tl[clip]]
        assert torch.equal(pr, flat[first:first + len(rows)]), f"chunk at row {first}"
    assert len(torch.unique(flat)) > 1
    assert torch.equal(eng.lin_scores(x, targets, bd, grid, sigma), scores)                 # two runs, the same bits
    frozen = eng.shap_scores(x, targets, 1, grid, sigma, SEED)[:, 0, P]
    e = rel_err_elem(scores[:, n].cpu().numpy(), frozen.cpu().numpy(), FLOOR)
    assert e < _gate(math)
    return e


def test_i3d_rows_equal_st_perturbed_forward(s16):
    x = _s16_x((21, 7))
    targets = s16.argmax(s16.forward(x)).tolist()
    e = _chain(s16, x, targets, (2, 2, 2), 0.0, 20, s16.math, "kshap")
    note(f"linsur chain I3D {s16.math}: 42 rows bit-equal to st_perturbed_forward; row n against Shapley's prefix P {e:.2e}")


@pytest.mark.parametrize("kind", ["kshap", "lime"])
def test_clstm_rows_equal_st_perturbed_forward(clstm, kind):
    eng, c = clstm
    e = _chain(eng, c['x'].cuda(), _tg(c), (3,) + SR.CHAIN_GRID, SR.CHAIN_SIGMA, 40, "fp32", kind)
    note(f"linsur chain ConvLSTM S2 {kind}: rows bit-equal to st_perturbed_forward; row n against Shapley's prefix P {e:.2e}")


KSHAP_OUT = {"kshap_scores", "kshap_cells", "kshap_total", "kshap_ok", "kshap_r2", "kshap_sizes", "score_x", "kshap_map",
             "kshap_frames"}
LIME_OUT = {"lime_scores", "lime_cells", "lime_intercept", "lime_ok", "lime_r2", "score_x", "lime_map", "lime_frames"}


def _check_fit(r, pre, Z, grid, wtab, ridge, what):
    """the engine's result against the numpy fit of its own scores, at the solve gate"""
    s, sx = r[pre + "_scores"].cpu().numpy(), r["score_x"].cpu().numpy()
    b = s.shape[0]
    fit = LR.kshap_fit(Z, s, sx) if pre == "kshap" else LR.lime_fit(Z, s, sx, wtab, ridge)
    assert not fit["singular"] and r[pre + "_ok"].cpu().tolist() == [1] * b and r[pre + "_ok"].dtype == torch.int32
    cells = r[pre + "_cells"].cpu().numpy().reshape(b, -1)
    assert tuple(r[pre + "_cells"].shape) == (b,) + tuple(grid)
    err, lim = np.abs(cells.astype(np.float64) - fit["cells"]), LR.gate(fit["cells"], fit["e_ref"])
    assert bool((err <= lim).all()), (what, float((err / lim).max()))
    icpt = r["lime_intercept"].cpu().numpy() if pre == "lime" else np.zeros(b, np.float32)
    want = LR.r2_ref(Z, fit["w"], s, sx, cells, icpt, fit["t"], fit["Wsum"]).astype(np.float32)
    assert np.array_equal(r[pre + "_r2"].cpu().numpy().view(np.uint32), want.view(np.uint32)), what
    if pre == "kshap":
        assert np.array_equal(r["kshap_total"].cpu().numpy(), fit["total"].astype(np.float32))
        gap = np.abs(cells.astype(np.float64).sum(axis=1) - fit["total"])
        assert bool((gap <= Z.shape[1] * 2.0 ** -24 * np.abs(cells.astype(np.float64)).sum(axis=1)).all())
    else:
        e0 = np.abs(icpt.astype(np.float64) - fit["intercept"])
        assert bool((e0 <= _icpt_gate(fit)).all())
    note(f"linsur fit {what}: cells err / gate {float((err / lim).max()):.3f}, r2 {r[pre + '_r2'].cpu().tolist()}")
    return fit


def _check_maps(eng, r, pre, grid, sigma):
    """the map and the frame profile are built from the cells exactly as shapley() builds its own"""
    gt, gh, gw = grid
    cells = r[pre + "_cells"]
    b, T = cells.shape[0], eng.clip_shape[1]
    kt = (np.arange(T) * gt) // T
    S = cells[:, torch.from_numpy(kt).cuda()].contiguous()
    assert torch.equal(r[pre + "_map"], eng.st_expand(S, (gh, gw), sigma))
    assert tuple(r[pre + "_map"].shape) == (b, T) + tuple(eng.clip_shape[2:]) and tuple(r[pre + "_frames"].shape) == (b, T)
    c64 = cells.cpu().numpy().astype(np.float64)
    fr = r[pre + "_frames"].cpu().numpy().astype(np.float64)
    assert bool((np.abs(fr.sum(axis=1) - c64.sum(axis=(1, 2, 3))) <= SH.frames_sum_bound(c64, grid)).all())


def test_clstm_kernelshap_and_lime_are_the_numpy_fit_of_their_scores(clstm):
    eng, c = clstm
    x, tg = c['x'].cuda(), _tg(c)
    grid, sigma = (3,) + SR.CHAIN_GRID, SR.CHAIN_SIGMA
    P = grid[0] * grid[1] * grid[2]
    r = eng.kernelshap(x, tg, n_samples=4 * P, grid=grid, sigma=sigma, seed=SEED)
    assert set(r) == KSHAP_OUT
    Z, s = LR.kshap_rows(SEED, 4 * P, P)
    assert np.array_equal(r["kshap_sizes"].cpu().numpy().astype(np.int64), s)
    bd, _ = eng.kshap_rows(4 * P, grid, SEED)
    assert torch.equal(r["kshap_scores"], eng.lin_scores(x, tg, bd, grid, sigma))
    idx = torch.arange(x.shape[0], device='cuda')
    assert torch.equal(r["score_x"], eng.forward(x)[idx, torch.as_tensor(tg, device='cuda')])
    _check_fit(r, "kshap", Z, grid, None, 0.0, "ConvLSTM S2 KernelSHAP")
    _check_maps(eng, r, "kshap", grid, sigma)
    again = eng.kernelshap(x, tg, n_samples=4 * P, grid=grid, sigma=sigma, seed=SEED)
    for k in KSHAP_OUT:
        assert torch.equal(bits(again[k]) if again[k].is_floating_point() else again[k],
                           bits(r[k]) if r[k].is_floating_point() else r[k]), k
    # b beyond max_batch: the same clips twice give the same rows twice, within the other-composition gate
    r4 = eng.kernelshap(torch.cat([x, x]), tg + tg, n_samples=4 * P, grid=grid, sigma=sigma, seed=SEED)
    for half in (r4["kshap_scores"][:2], r4["kshap_scores"][2:]):
        assert rel_err_elem(half.cpu().numpy(), r["kshap_scores"].cpu().numpy(), FLOOR) < _gate("fp32")
    # LIME
    rl = eng.lime(x, tg, n_samples=60, p=0.5, grid=grid, sigma=sigma, seed=SEED, width=0.25, ridge=1.0)
    assert set(rl) == LIME_OUT
    Zl = LR.lime_rows(SEED, RR.thresh(0.5), 60, P)
    assert torch.equal(rl["lime_scores"], eng.lin_scores(x, tg, eng.lime_rows(60, 0.5, grid, SEED), grid, sigma))
    _check_fit(rl, "lime", Zl, grid, LR.lime_wtab(P, 0.25), 1.0, "ConvLSTM S2 LIME")
    _check_maps(eng, rl, "lime", grid, sigma)
    other = eng.lime(x, tg, n_samples=60, p=0.5, grid=grid, sigma=sigma, seed=SEED, width=0.5, ridge=0.25)
    assert torch.equal(other["lime_scores"], rl["lime_scores"]) and not torch.equal(other["lime_cells"], rl["lime_cells"])
    # the default grid: the frames
    T = x.shape[2]
    rd = eng.kernelshap(x, tg, n_samples=4 * T)
    assert tuple(rd["kshap_cells"].shape) == (2, T, 1, 1) and rd["kshap_ok"].cpu().tolist() == [1, 1]
    assert np.array_equal(rd["kshap_frames"].cpu().numpy(), rd["kshap_cells"].cpu().numpy().reshape(2, T))   # one frame a cell


def test_i3d_kernelshap_and_lime_are_the_numpy_fit_of_their_scores(s16):
    x = _s16_x()
    t = s16.argmax(s16.forward(x)).tolist()
    grid = (2, 2, 2)
    r = s16.kernelshap(x, t, n_samples=32, grid=grid, sigma=0.0, seed=SEED)
    _check_fit(r, "kshap", LR.kshap_rows(SEED, 32, 8)[0], grid, None, 0.0, f"I3D {s16.math} KernelSHAP")
    _check_maps(s16, r, "kshap", grid, 0.0)
    rl = s16.lime(x, t, n_samples=32, grid=grid, sigma=0.0, seed=SEED)
    _check_fit(rl, "lime", LR.lime_rows(SEED, RR.thresh(0.5), 32, 8), grid, LR.lime_wtab(8), 1.0, f"I3D {s16.math} LIME")
    _check_maps(s16, rl, "lime", grid, 0.0)


# ---------------------------------------------------------------------------------------------------- F. fixture
def test_s16_scores_and_fits_vs_fixture(s16, golden):
    """the 65 rows of tests/golden/linsur.npz within 1e-3 relative, each against its own magnitude (the gate of
    test_gpu_shapley.py on shapley.npz); target bit-exact; the device's fit of the FIXTURE's scores against the
    fixture's fp64 cells at the solve gate"""
    g = golden('linsur')
    grid, n, seed = tuple(int(v) for v in g['grid']), int(g['n']), int(g['seed'])
    assert (grid, n, seed, int(g['paired']), float(g['sigma']), int(g['clip'])) == ((2, 2, 2), 32, 1234, 1, 0.0, 21)
    Zk, sk = LR.kshap_rows(seed, n, 8)
    Zl = LR.lime_rows(seed, RR.thresh(float(g['p'])), n, 8)
    assert np.array_equal(g['kshap_rows'], Zk) and np.array_equal(g['kshap_sizes'], sk) and np.array_equal(g['lime_rows'], Zl)
    x = _s16_x()
    t = int(torch.argmax(s16.forward(x)[0]))
    assert t == int(g['target'])                                    # integer output: bit-exact
    rk = s16.kernelshap(x, [t], n_samples=n, grid=grid, sigma=0.0, seed=seed)
    rl = s16.lime(x, [t], n_samples=n, p=float(g['p']), grid=grid, sigma=0.0, seed=seed, width=float(g['width']),
                  ridge=float(g['ridge']))
    ek = rel_err_elem(rk["kshap_scores"][0].cpu().numpy(), g['kshap_scores'], FLOOR)
    el = rel_err_elem(rl["lime_scores"][0].cpu().numpy(), g['lime_scores'], FLOOR)
    eo = abs(float(rk["score_x"][0]) - float(g['orig']))
    assert ek < 1e-3 and el < 1e-3 and eo < 1e-3 * float(g['orig'])
    # the fit, on the fixture's own scores
    orig = torch.from_numpy(np.asarray(g['orig'], np.float32).reshape(1)).cuda()
    worst = {}
    for pre, Z, sc, wtab, ridge in (("kshap", Zk, g['kshap_scores'], None, 0.0),
                                    ("lime", Zl, g['lime_scores'], LR.lime_wtab(8, float(g['width'])), float(g['ridge']))):
        fit = s16.lin_solve("kernelshap" if pre == "kshap" else "lime", torch.from_numpy(sc[None]).cuda(), orig,
                            _dev_bits(Z), 8, wtab, ridge)
        ref = LR.kshap_fit(Z, sc[None], g['orig'].reshape(1)) if pre == "kshap" else \
            LR.lime_fit(Z, sc[None], g['orig'].reshape(1), wtab, ridge)
        want = g[pre + '_cells'].reshape(1, 8)
        assert float(np.abs(ref["cells"] - want).max()) <= 1e-12 * float(np.abs(want).max())     # the fixture is the reference's fit
        err = np.abs(fit["cells"].cpu().numpy().astype(np.float64) - want)
        lim = LR.gate(want, ref["e_ref"])
        worst[pre] = float((err / lim).max())
        assert bool((err <= lim).all()) and fit["ok"].cpu().tolist() == [1]
    assert abs(float(fit["intercept"][0]) - float(g['lime_intercept'])) <= float(_icpt_gate(ref)[0])      # the LIME pass came last
    note(f"linsur scores vs fixture {s16.math}: 65 rows, elementwise rel kshap {ek:.2e} lime {el:.2e}, orig {eo:.2e} abs; "
         f"fit of the fixture's scores err / gate kshap {worst['kshap']:.3f} lime {worst['lime']:.3f}")


# ---------------------------------------------------------------------------------------------------- G. surfaces
def test_surrogate_videos_i3d(smth_model):
    import ivf_recipe as RC
    from linear_surrogate_videos import KernelShapVideo, LimeVideo
    x = torch.from_numpy(RC.clip(21))[None]
    kv = KernelShapVideo(smth_model, n_samples=64, seed=3)                # the default grid: 16 frames, 65 rows
    m, out = kv(x)
    assert m.shape == (16, 224, 224) and m.dtype == np.float32 and tuple(out.shape) == (1, 174)
    assert np.isfinite(m).all() and m.any() and set(kv.last) == KSHAP_OUT
    assert tuple(kv.last["kshap_cells"].shape) == (1, 16, 1, 1) and tuple(kv.last["kshap_scores"].shape) == (1, 65)
    eng = smth_model._engine_for(x.cuda(), min_batch=32)
    pred = int(torch.argmax(out[0]))
    want = eng.kernelshap(x.cuda(), [pred], n_samples=64, seed=3)["kshap_map"][0].cpu().numpy()
    # 32 paired rows of seed 3 on 16 players are a singular sample (rank 14 of 15): refused by the pivot rule, loudly
    sing = eng.kernelshap(x.cuda(), [pred], n_samples=32, seed=3)
    assert sing["kshap_ok"].cpu().tolist() == [0] and bool(torch.isnan(sing["kshap_cells"]).all())
    assert bool(torch.isnan(sing["kshap_r2"]).all()) and bool(torch.isfinite(sing["kshap_scores"]).all())
    assert np.array_equal(m.view(np.uint32), want.view(np.uint32))           # index None = the argmax; two runs, same bits
    lv = LimeVideo(smth_model, n_samples=24, grid=(2, 2, 2), seed=3)
    m3, _ = lv(x, index=3)
    assert m3.shape == (16, 224, 224) and m3.dtype == np.float32 and np.isfinite(m3).all() and set(lv.last) == LIME_OUT
    assert tuple(lv.last["lime_cells"].shape) == (1, 2, 2, 2) and tuple(lv.last["lime_scores"].shape) == (1, 25)


def test_surrogate_videos_clstm():
    import ivf_lib as L
    import ivf_recipe as RC
    from linear_surrogate_videos import KernelShapVideo, LimeVideo
    model = _kth_clstm()
    x = torch.from_numpy(RC.clip(7, 3, 32, 120, 160))[None]
    kv = KernelShapVideo(model, n_samples=16, grid=(4, 1, 2), seed=1, paired=False, archType="CLSTM")
    m, out = kv(x, index=2)
    assert m.shape == (32, 120, 160) and m.dtype == np.float32 and tuple(out.shape) == (1, 6)
    assert tuple(kv.last["kshap_cells"].shape) == (1, 4, 1, 2) and tuple(kv.last["kshap_scores"].shape) == (1, 17)
    m2, _ = LimeVideo(model, n_samples=16, grid=(4, 1, 2), seed=1, archType="CLSTM")(x, index=2)
    assert m2.shape == (32, 120, 160)
    with pytest.raises(L.IvfError):
        KernelShapVideo(model, archType="VGG")(x)
    with pytest.raises(L.IvfError):
        LimeVideo(model, archType="CLSTM")(torch.cat([x, x]))


def test_refusals(clstm):
    import ivf_engine
    import ivf_lib as L
    eng, c = clstm
    x, tg = c['x'].cuda(), _tg(c)
    T = x.shape[2]
    for grid in ((T + 1, 3, 4), (0, 3, 4), (3, 33, 4), (3, 3, 0), (3, 4), "abc", (1, 1, 1), (5, 15, 15), (2, 32, 32)):
        for call in (lambda: eng.kernelshap(x, tg, n_samples=4096, grid=grid), lambda: eng.lime(x, tg, n_samples=8, grid=grid),
                     lambda: eng.kshap_rows(8, grid=grid), lambda: eng.lime_rows(8, grid=grid)):
            with pytest.raises(L.IvfError):
                call()
    g = (3, 3, 4)
    for kw in (dict(n_samples=34), dict(n_samples=37), dict(n_samples=2 ** 20 + 2), dict(n_samples=0), dict(n_samples=40, seed=-1)):
        with pytest.raises(L.IvfError):                                # < P - 1; odd with paired; too many; none; seed
            eng.kernelshap(x, tg, grid=g, **kw)
    eng.kshap_rows(37, g, paired=False)                                # an odd count is fine without the pairing
    for kw in (dict(p=0.0), dict(p=1.0), dict(width=0.0), dict(ridge=-1.0), dict(n_samples=2 ** 20 + 1), dict(width="x")):
        with pytest.raises(L.IvfError):
            eng.lime(x, tg, grid=g, **{"n_samples": 8, **kw})
    with pytest.raises(L.IvfError):
        eng.kernelshap(x, tg[:1], n_samples=40, grid=g)                  # one target for two clips
    bd, _ = eng.kshap_rows(40, g)
    with pytest.raises(L.IvfError):
        eng.lin_scores(x, tg, bd, (3, 3, 3))                             # 27 players: one word, not two
    with pytest.raises(L.IvfError):
        eng.lin_scores(x, tg, bd.long(), g)
    with pytest.raises(L.IvfError):
        eng.lin_solve("kernelshap", torch.zeros(2, 40, device='cuda'), torch.zeros(2, device='cuda'), bd, 36)   # 40 is not n + 1
    with pytest.raises(L.IvfError):
        eng.lin_solve("shap", torch.zeros(2, 41, device='cuda'), torch.zeros(2, device='cuda'), bd, 36)
    # the C entry: null pointers and a bad grid come back as error codes, nothing is written
    lib = L.lib()
    _, _, _, AH, AW = eng._st_axes((3, 4), 1.0)
    sc = torch.full((2, 41), -12345.0, device='cuda')
    tgt = torch.as_tensor(tg, dtype=torch.int32, device='cuda')
    fn = lib.ivf_clstm_lin_scores
    assert fn(eng._h, None, 2, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 3, 4, 40, L.ptr(bd), L.ptr(sc), L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 2, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 3, 4, 40, None, L.ptr(sc), L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 2, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 3, 4, 40, L.ptr(bd), None, L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 0, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 3, 4, 40, L.ptr(bd), L.ptr(sc), L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 2, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 3, 4, 0, L.ptr(bd), L.ptr(sc), L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 2, L.ptr(tgt), L.ptr(AH), L.ptr(AW), T + 1, 3, 4, 40, L.ptr(bd), L.ptr(sc), L.stream()) == -1
    assert b"lin_" in lib.ivf_last_error()
    assert lib.ivf_lin_stage(L.ptr(x), 2, 2, T, 24, 32, L.ptr(AH), L.ptr(AW), 2, 32, 32, 40, L.ptr(bd), 0, 1, L.ptr(sc), 0,
                             L.stream()) == -1 and b"lin_stage" in lib.ivf_last_error()      # 2048 players
    torch.cuda.synchronize()
    assert bool((sc == -12345.0).all())
    # the TF-style plan has no such entry and refuses
    tf = ivf_engine.TFCLSTMEngine(5, (1, 8, 30, 40), units=(4,), kernel=(3, 5), stride=2, padding="valid", max_batch=1)
    assert not hasattr(lib, "ivf_tfclstm_lin_scores")
    xt = torch.zeros(1, 1, 8, 30, 40, device='cuda')
    for call in (lambda: tf.kernelshap(xt, [0], n_samples=8, grid=(2, 2, 2)), lambda: tf.lime(xt, [0], n_samples=8, grid=(2, 2, 2)),
                 lambda: tf.kshap_rows(8, grid=(2, 2, 2)), lambda: tf.lime_rows(8, grid=(2, 2, 2))):
        with pytest.raises(L.IvfError):
            call()


KSHAP_KEYS = {'true_class', 'pred_class', 'video_id', 'KshapHeatMap', 'KshapCells', 'KshapFrames', 'kshap_total', 'kshap_ok',
              'kshap_r2', 'n_samples', 'seed'}
LIME_KEYS = {'true_class', 'pred_class', 'video_id', 'LimeHeatMap', 'LimeCells', 'LimeFrames', 'lime_intercept', 'lime_ok',
             'lime_r2', 'n_samples', 'seed'}


def test_smth_driver_with_kernelshap_lime_and_curves(smth_model, tmp_path, monkeypatch):
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    import ivf_lib as L
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    loader = ivf_find_masks.SyntheticLoader(2, 2, (3, 16, 224, 224), 174, first_id=40)
    hp = {"batch_size": 2, "gradCamType": "guessed"}
    drv.find_masks(loader, smth_model, hp, 0.01, 0.02, 2, "central", "freeze", classOI=None, doGradCam=False,
                   runTempMask=True, verbose=False, doKernelShap=True, kshapSamples=16, kshapGrid=(2, 2, 2), kshapSeed=5,
                   doLime=True, limeSamples=24, limeGrid=(2, 2, 2), limeSeed=6, doCurves=True, curveGrid=(2, 2, 2))
    tm = pickle.load(open(tmp_path / "results" / "allTimeMaskResults_run0_None_.p", "rb"))
    ks = pickle.load(open(tmp_path / "results" / "allKernelShapResults_run0_None_.p", "rb"))
    lm = pickle.load(open(tmp_path / "results" / "allLimeResults_run0_None_.p", "rb"))
    cv = pickle.load(open(tmp_path / "results" / "allCurvesResults_run0_None_.p", "rb"))
    assert len(ks) == len(lm) == len(tm) == len(cv) == 2
    for rec, lrec, trec, crec in zip(ks, lm, tm, cv):
        assert set(rec) == KSHAP_KEYS and set(lrec) == LIME_KEYS
        assert rec['KshapHeatMap'].shape == (16, 224, 224) and rec['KshapHeatMap'].dtype == np.float32
        assert rec['KshapCells'].shape == (2, 2, 2) and rec['KshapFrames'].shape == (16,)
        assert lrec['LimeHeatMap'].shape == (16, 224, 224) and lrec['LimeCells'].shape == (2, 2, 2)
        assert rec['pred_class'] == trec['pred_class'] == lrec['pred_class']
        assert (rec['n_samples'], rec['seed'], lrec['n_samples'], lrec['seed']) == (16, 5, 24, 6)
        assert rec['kshap_ok'] == 1 and lrec['lime_ok'] == 1 and np.isfinite(rec['KshapCells']).all()
        assert isinstance(rec['kshap_total'], float) and isinstance(lrec['lime_intercept'], float)
        assert abs(float(rec['KshapCells'].astype(np.float64).sum()) - rec['kshap_total']) <= 2.0 ** -24 * \
            (8 * float(np.abs(rec['KshapCells']).astype(np.float64).sum()) + abs(rec['kshap_total']))      # efficiency
        assert crec['grid'] == (2, 2, 2) and {'kshap', 'lime'} <= set(crec)      # the curves table ranks both
        assert crec['kshap']['deletion'].shape == (9,) and np.isfinite(crec['lime']['del_auc'])
    assert ks[0]['video_id'] == 40
    last = ivf_find_masks.find_masks_impl.last_kshap_results
    assert len(last) == 2 and all(np.array_equal(a['KshapHeatMap'], q['KshapHeatMap']) for a, q in zip(last, ks))
    assert len(ivf_find_masks.find_masks_impl.last_lime_results) == 2
    assert not (tmp_path / "results" / "allShapleyResults_run0_None_.p").exists()
    for folder in ("kernelshap", "lime"):
        strips = [q for q in (tmp_path / "cam_saved_images").rglob(folder + "/*.png")]
        assert any(q.name == "casefreeze40_15.png" for q in strips), folder
    with pytest.raises(L.IvfError):
        drv.find_masks(loader, smth_model, hp, 0.01, 0.02, 2, "central", "reverse", classOI=None, doGradCam=False,
                       runTempMask=True, verbose=False, doKernelShap=True, kshapSamples=16, kshapGrid=(2, 2, 2))
    with pytest.raises(L.IvfError):
        drv.find_masks(loader, smth_model, hp, 0.01, 0.02, 2, "central", "reverse", classOI=None, doGradCam=False,
                       runTempMask=True, verbose=False, doLime=True, limeSamples=16, limeGrid=(2, 2, 2))
