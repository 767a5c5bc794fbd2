"""Deletion / insertion curves (csrc/curve_ops.hip) on the GPU: the per-clip rank table against the
numpy restatement (equality), the pooled cells against fp64 within the derived bound, the staging kernel against
ivf_shap_stage with the same table and against ivf_stmask_expand_fwd + ivf_stfreeze_fwd on each row's explicit S
(equality), the score rows on both plans against ivf_*_shap_scores and st_perturbed_forward (equality) and against
tests/golden/curves.npz (make_golden_curves.py: the reference's I3D under the torch restatement of expand and per-pixel
freeze), the reduction against fp64 and the derived bounds of tests/curve_refs.py, and the public surfaces.
tests/test_curve_refs_host.py proves the references on the CPU."""
import pickle

import numpy as np
import pytest
import torch

import box_refs as B
import curve_refs as CR
import shap_refs as SH
import stmask_refs as SR
from conftest import note, rel_err_elem
from test_gpu_box import FLOOR, _gate
from test_gpu_leaf_kernels import bits, guarded, untouched
from test_gpu_shapley import _kth_clstm, _s16_x, _tg, clstm, s16, smth_model  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00ABC
U = CR.U


def _dev_ranks(rk):
    """a numpy rank table as the int16 device tensor the entries take (uint16 values below 4096)"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(rk).astype(np.int16))).cuda().contiguous()


def _planted(b, shape, seed):
    """float32 [b, *shape] with many ties, NaNs, both zeros and both infinities"""
    g = np.random.default_rng(seed)
    a = (g.integers(-6, 7, (b,) + tuple(shape)) / 4.0).astype(np.float32)
    a[g.random(a.shape) < 0.1] = np.nan
    a[g.random(a.shape) < 0.1] = -0.0
    a.reshape(b, -1)[0, 0] = np.inf
    a.reshape(b, -1)[-1, -1] = -np.inf
    return a


# ---------------------------------------------------------------------------------------------------- A. rank table
def _ranks(a, T, grid, order):
    import ivf_lib as L
    b, t_in = a.shape[:2]
    P = grid[0] * grid[1] * grid[2]
    buf, rk = guarded((b, P), dtype=torch.int16, sent=-77)
    rk.fill_(0x7ABC)
    ad = torch.from_numpy(a).cuda().contiguous()
    L.check(L.lib().ivf_curve_ranks(L.ptr(ad), b, t_in, T, *grid, order, L.ptr(rk), L.stream()))
    torch.cuda.synchronize()
    assert untouched(buf, -77)
    return rk.cpu().numpy().astype(np.int64) & 0xFFFF


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("grid", [(9, 1, 1), (2, 2, 2), (3, 5, 7), (4, 32, 32)])
def test_rank_table_is_the_restatement(grid, order):
    b, P = 3, grid[0] * grid[1] * grid[2]
    a = _planted(b, grid, 11 + P)
    got = _ranks(a, max(grid[0], 9), grid, order)
    assert np.array_equal(got, CR.ranks(a.reshape(b, P), order)), (grid, order)
    assert np.array_equal(np.sort(got, axis=1), np.broadcast_to(np.arange(P), (b, P)))
    # a clip's table does not depend on the other clips
    assert np.array_equal(_ranks(a[1:2], max(grid[0], 9), grid, order), got[1:2])


def test_rank_known_answers_on_the_device():
    a = np.array([[0.5, 2.0, -1.0, 2.0, 0.5, np.nan, -0.0, 0.0]], np.float32).reshape(1, 8, 1, 1)
    assert _ranks(a, 8, (8, 1, 1), 0)[0].tolist() == [2, 0, 6, 1, 3, 7, 4, 5]
    assert _ranks(a, 8, (8, 1, 1), 1)[0].tolist() == [3, 5, 0, 6, 4, 7, 1, 2]


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("gh,gw", [(1, 1), (2, 3)])
def test_ranks_of_per_frame_cells_average_uneven_temporal_cells(gh, gw, order):
    """t_in = T = 9, gt = 4: temporal cells of 3, 2, 2, 2 frames; and t_in = gt on the same means gives the same table"""
    b, T, gt = 3, 9, 4
    a = _planted(b, (T, gh, gw), 5)
    a[np.isinf(a)] = 1.0                                  # inf - inf inside a mean is a NaN of either sign bit: keep it out
    cells = CR.grid_cells(a, T, gt)
    want = CR.ranks(cells.reshape(b, -1), order)
    assert np.array_equal(_ranks(a, T, (gt, gh, gw), order), want)
    assert np.array_equal(_ranks(cells, T, (gt, gh, gw), order), want)
    assert np.isnan(cells).any() and not np.isnan(cells).all()


def test_pooled_cells_and_their_ranks(clstm):
    """a [b,T,H,W] map pooled to the footprint-weighted mean: against fp64 within (H W + T + 3) u sum|terms| / den; the
    ranks against the restatement applied to the DEVICE's cells (exact), never against fp64 ranks"""
    eng, c = clstm
    C, T, H, W = eng.clip_shape
    b = 2
    g = np.random.default_rng(21)
    a = (g.standard_normal((b, T, H, W)) * 3).astype(np.float32)
    ad = torch.from_numpy(a).cuda()
    for (gh, gw), sigma in (((3, 4), 1.0), ((2, 2), 0.0), ((1, 1), None)):
        cells = eng.curve_cells(ad, (T, gh, gw), sigma)
        assert tuple(cells.shape) == (b, T, gh, gw)
        _, _, _, AH, AW = eng._st_axes((gh, gw), sigma)
        want, mag, den = CR.pool_ref(a, AH.cpu().numpy(), AW.cpu().numpy())
        err = np.abs(cells.cpu().numpy().astype(np.float64) - want)
        bound = (H * W + T + 3) * U * mag
        note(f"curve pooling {(gh, gw)} sigma {sigma}: worst err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
        for gt in (T, 4):
            for order in ("morf", "lerf"):
                rk = eng.curve_ranks(ad, (gt, gh, gw), sigma, order).cpu().numpy().astype(np.int64) & 0xFFFF
                dev_cells = CR.grid_cells(cells.cpu().numpy(), T, gt).reshape(b, -1)
                assert np.array_equal(rk, CR.ranks(dev_cells, 0 if order == "morf" else 1))


# ---------------------------------------------------------------------------------------------------- B. staging
def _stage(xd, AHd, AWd, dims, rkd, curves, step, first, count, cpad):
    import ivf_lib as L
    b, C, T, H, W, (gt, gh, gw) = dims
    buf, out = guarded((count, C, T, H * W) if cpad == 0 else (count, T, H * W, 4))
    bits(out).fill_(NAN_BITS)
    L.check(L.lib().ivf_curve_stage(L.ptr(xd), b, C, T, H, W, L.ptr(AHd), L.ptr(AWd), gt, gh, gw, L.ptr(rkd), curves, step,
                                    first, count, L.ptr(out), cpad, L.stream()))
    torch.cuda.synchronize()
    assert untouched(buf), f"curve_stage out_cpad={cpad}: a sentinel row was written"
    assert not bool(torch.isnan(out).any()), f"curve_stage out_cpad={cpad}: an element was never written"
    return out


def _pair(xd, AHd, AWd, dims, rk, rows, cpad):
    """the rows [(clip, ins, k)] by ivf_stmask_expand_fwd + ivf_stfreeze_fwd on the explicit per-frame S"""
    import ivf_lib as L
    b, C, T, H, W, grid = dims
    gt, gh, gw = grid
    count = len(rows)
    S = torch.from_numpy(CR.frame_masks(CR.row_masks(rk, grid, rows), T)).cuda().contiguous()         # [count,T,gh,gw]
    xr = xd[torch.tensor([r[0] for r in rows]).cuda()].contiguous()
    M = torch.empty(count, T, H, W, device='cuda')
    L.check(L.lib().ivf_stmask_expand_fwd(L.ptr(S), L.ptr(AHd), L.ptr(AWd), L.ptr(M), count, T, gh, gw, H, W, L.stream()))
    out = torch.empty((count, C, T, H * W) if cpad == 0 else (count, T, H * W, 4), device='cuda')
    L.check(L.lib().ivf_stfreeze_fwd(L.ptr(xr), L.ptr(M), L.ptr(out), count, C, T, H * W, cpad, L.stream()))
    torch.cuda.synchronize()
    return out


def _shap_rows(xd, AHd, AWd, dims, rk, cpad):
    """{(clip, ins): the P + 1 rows of ivf_shap_stage at b = 1, n = 1}: the clip's table for deletion, the reversed
    table for insertion (insertion at k under rank == prefix P - k under P - 1 - rank)"""
    import ivf_lib as L
    b, C, T, H, W, (gt, gh, gw) = dims
    P = gt * gh * gw
    out = {}
    for cl in range(b):
        for ins in (0, 1):
            tab = _dev_ranks((P - 1 - rk[cl]) if ins else rk[cl])
            o = torch.empty((P + 1, C, T, H * W) if cpad == 0 else (P + 1, T, H * W, 4), device='cuda')
            xc = xd[cl:cl + 1].contiguous()
            L.check(L.lib().ivf_shap_stage(L.ptr(xc), 1, C, T, H, W, L.ptr(AHd), L.ptr(AWd), gt, gh, gw, 1, L.ptr(tab), 0,
                                           P + 1, L.ptr(o), cpad, L.stream()))
            out[(cl, ins)] = o
    torch.cuda.synchronize()
    return out


def _windows(b, per):
    """inside the first curve, across the curve boundary, across the clip boundary, ending on the last row, the whole"""
    tot = b * per
    return [(1, 5), (per // 2 - 3, 7) if per >= 8 else (0, per), (per - 4, 9), (tot - 5, 5), (0, tot)]


def _check_stage(C, T, sigma, grid, cpad, H=12, W=20, b=2, combos=((3, 1), (3, 3), (1, 1), (2, 3), (1, 3), (2, 1))):
    gt, gh, gw = grid
    P = gt * gh * gw
    dims = (b, C, T, H, W, grid)
    xd = B.stage_inputs(b, C, T, H, W, key='curve').cuda()
    AHd, AWd = SR.axis_weights(H, gh, sigma).cuda(), SR.axis_weights(W, gw, sigma).cuda()
    g = np.random.default_rng(P + T)
    rk = np.stack([g.permutation(P) for _ in range(b)])             # a different table per clip
    assert not np.array_equal(rk[0], rk[1])
    rkd = _dev_ranks(rk)
    shap = _shap_rows(xd, AHd, AWd, dims, rk, cpad)
    moved = 0
    for curves, step in combos:
        rows = CR.row_list(b, P, step, curves)
        per = len(rows) // b
        for first, count in _windows(b, per):
            first, count = max(first, 0), min(count, b * per - max(first, 0))
            win = rows[first:first + count]
            got = _stage(xd, AHd, AWd, dims, rkd, curves, step, first, count, cpad)
            what = f"curves {curves} step {step} rows [{first}, {first + count}) of {b * per}"
            assert torch.equal(got, _pair(xd, AHd, AWd, dims, rk, win, cpad)), what + ": not expand_fwd + stfreeze_fwd"
            want = torch.stack([shap[(cl, ins)][(P - k) if ins else k] for cl, ins, k in win])
            assert torch.equal(bits(got), bits(want)), what + ": not the bits of ivf_shap_stage with the same table"
            if cpad == 4:
                assert torch.equal(bits(got[..., C:]), torch.zeros_like(bits(got[..., C:]))), "pad lane not +0.0"
            src = xd[torch.tensor([r[0] for r in win]).cuda()].reshape(count, C, T, H * W)
            flat = got if cpad == 0 else got[..., :C].permute(0, 3, 1, 2)
            moved += int((flat != src).any(dim=(1, 2, 3)).sum())
    assert moved > 0, "no staged row differs from its clip: the comparison is vacuous"


@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("sigma", [0.0, 1.5])
@pytest.mark.parametrize("C", [1, 3])
def test_staging_is_shap_stage_and_expand_plus_freeze(C, sigma, cpad):
    """b = 2, T = 9, 12 x 20 (one workgroup with 16 idle threads), grid (3, 3, 4): P = 36; step 1 (37 rows a curve) and
    step 3 (13 rows), curves 1, 2, 3, windows across curve and clip boundaries"""
    _check_stage(C, 9, sigma, (3, 3, 4), cpad)


@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("T", [16, 32])
def test_staging_on_the_exact_frame_count_paths(T, cpad):
    """T = 16 and 32: pieces of 16 preloaded frames in the channels-last kernel; four temporal cells and one per frame"""
    _check_stage(3, T, 1.5, (4, 1, 2), cpad, combos=((3, 1), (3, 3)))
    _check_stage(3, T, 0.0, (T, 1, 1), cpad, combos=((3, 3), (2, 1)))


@pytest.mark.parametrize("cpad", [0, 4])
def test_staging_over_several_workgroups(cpad):
    """23 x 27 = 621 pixels: three workgroups per row, the last ragged; the widest grid row (32 cells: bit 31)"""
    _check_stage(3, 9, 1.0, (2, 4, 5), cpad, H=23, W=27, combos=((3, 3), (3, 1)))
    _check_stage(2, 3, 0.7, (3, 2, 32), cpad, H=9, W=40, combos=((3, 7),))


# ---------------------------------------------------------------------------------------------------- C. plans
def _shap_rows_on_plan(eng, x1, t1, grid, sigma, table):
    """ivf_*_shap_scores of one clip, one permutation, the caller's table: [P + 1]"""
    import ivf_lib as L
    gt, gh, gw = grid
    _, _, _, AH, AW = eng._st_axes((gh, gw), sigma)
    tg = torch.as_tensor([t1], dtype=torch.int32, device='cuda')
    sc = torch.empty(1, 1, gt * gh * gw + 1, device='cuda')
    L.check(eng._fn("shap_scores")(eng._h, L.ptr(x1), 1, L.ptr(tg), L.ptr(AH), L.ptr(AW), gt, gh, gw, 1,
                                   L.ptr(_dev_ranks(table)), L.ptr(sc), L.stream()))
    torch.cuda.synchronize()
    return sc[0, 0]


def _plan_checks(eng, x, targets, grid, sigma, step, math, what):
    b, T = x.shape[0], x.shape[2]
    P = grid[0] * grid[1] * grid[2]
    g = np.random.default_rng(P)
    rk = np.stack([g.permutation(P) for _ in range(b)])
    rkd = _dev_ranks(rk)
    # 1. one clip, one curve, step 1: the rows of ivf_*_shap_scores with the same table, in the same chunks (equality)
    x0 = x[:1].contiguous()
    dele = eng.curve_scores(x0, targets[:1], rkd[:1], grid, sigma, 1, 1)
    assert tuple(dele.shape) == (1, 1, P + 1)
    assert torch.equal(bits(dele[0, 0]), bits(_shap_rows_on_plan(eng, x0, targets[0], grid, sigma, rk[0])))
    ins = eng.curve_scores(x0, targets[:1], rkd[:1], grid, sigma, 1, 2)
    rev = _shap_rows_on_plan(eng, x0, targets[0], grid, sigma, P - 1 - rk[0]).flip(0)
    e_ins = rel_err_elem(ins[0, 0].cpu().numpy(), rev.cpu().numpy(), FLOOR)       # the same rows at other chunk places
    assert e_ins < _gate(math)
    assert len(torch.unique(dele)) > 2
    # 2. both curves: the ends, and every row == st_perturbed_forward of the explicit masks in the same chunk composition
    both = eng.curve_scores(x, targets, rkd, grid, sigma, step, 3)
    J = -(-P // step)
    assert tuple(both.shape) == (b, 2, J + 1)
    assert torch.equal(bits(both[:, 0, 0]), bits(both[:, 1, J])), "del[0] != ins[J]: the clip"
    assert torch.equal(bits(both[:, 0, J]), bits(both[:, 1, 0])), "del[J] != ins[0]: the fully frozen clip"
    rows = CR.row_list(b, P, step, 3)
    flat = both.reshape(-1)
    tl = torch.as_tensor(targets, device='cuda').long()
    Bp = eng.max_batch
    for first in range(0, len(rows), Bp):
        win = rows[first:first + Bp]
        S = torch.from_numpy(CR.frame_masks(CR.row_masks(rk, grid, win), T)).cuda().contiguous()
        clip = torch.tensor([r[0] for r in win]).cuda()
        M = eng.st_expand(S, grid[1:], sigma)
        pr = eng.st_perturbed_forward(x[clip].contiguous(), M)[torch.arange(len(win), device='cuda'), tl[clip]]
        assert torch.equal(bits(pr), bits(flat[first:first + len(win)])), f"chunk at row {first}"
    # 3. a clip's rows do not depend on the other clips of the call or on where the chunks fall
    one = eng.curve_scores(x[1:].contiguous(), list(targets[1:]), rkd[1:], grid, sigma, step, 3)
    e = rel_err_elem(both[1:].cpu().numpy(), one.cpu().numpy(), FLOOR)
    assert e < _gate(math)
    sx = eng.forward(x)[torch.arange(b, device='cuda'), tl].cpu().numpy()
    e_x = rel_err_elem(both[:, 0, 0].cpu().numpy(), sx, FLOOR)
    assert e_x < _gate(math)
    note(f"curve scores {what}: deletion rows bit-equal to shap_scores; insertion vs reversed table {e_ins:.2e}; "
         f"{len(rows)} rows bit-equal to st_perturbed_forward; clip 1 alone {e:.2e}; row 0 vs forward {e_x:.2e}")
    return both, rk


def test_i3d_scores(s16):
    x = _s16_x((21, 7))
    t = s16.argmax(s16.forward(x)).tolist()
    _plan_checks(s16, x, t, (2, 2, 2), 0.0, 3, s16.math, f"I3D {s16.math}")       # 2 clips x 2 curves x 4 rows


def test_clstm_scores(clstm):
    eng, c = clstm
    _plan_checks(eng, c['x'].cuda(), _tg(c), (3,) + SR.CHAIN_GRID, SR.CHAIN_SIGMA, 5, "fp32", "ConvLSTM S2")


def test_faithfulness_beyond_max_batch_and_its_pieces(clstm):
    eng, c = clstm
    x, tg = c['x'].cuda(), _tg(c)
    b, T = x.shape[0], x.shape[2]
    x4, tg4 = torch.cat([x, x]), tg + tg
    assert x4.shape[0] > eng.max_batch
    g = np.random.default_rng(0)
    attr = torch.from_numpy(g.standard_normal((2 * b, T)).astype(np.float32)).cuda()
    attr[b:] = attr[:b]
    r = eng.faithfulness(x4, tg4, attr)                                          # the default grid: the frames
    assert set(r) == {"curve_ranks", "del_scores", "ins_scores", "del_auc", "ins_auc", "del_auc_norm", "ins_auc_norm",
                      "score_x"}
    assert tuple(r["curve_ranks"].shape) == (2 * b, T) and tuple(r["del_scores"].shape) == (2 * b, T + 1)
    assert np.array_equal(r["curve_ranks"].cpu().numpy(), CR.ranks(attr.cpu().numpy(), 0))
    for k in ("del_scores", "ins_scores"):
        assert rel_err_elem(r[k][:b].cpu().numpy(), r[k][b:].cpu().numpy(), FLOOR) < _gate("fp32")
    sc = eng.curve_scores(x4, tg4, r["curve_ranks"], None, None, 1, 3)
    assert torch.equal(bits(sc[:, 0]), bits(r["del_scores"])) and torch.equal(bits(sc[:, 1]), bits(r["ins_scores"]))
    auc, norm = eng.curve_reduce(sc)
    assert torch.equal(bits(auc[:, 0]), bits(r["del_auc"])) and torch.equal(bits(norm[:, 1]), bits(r["ins_auc_norm"]))
    ref = CR.auc_ref(sc.cpu().numpy(), T, 1, 3)
    assert bool((np.abs(auc.cpu().numpy() - ref["auc"]) <= ref["bound_auc"]).all())
    lerf = eng.faithfulness(x4, tg4, attr, order="lerf")
    assert np.array_equal(lerf["curve_ranks"].cpu().numpy(), T - 1 - r["curve_ranks"].cpu().numpy())    # no ties


# ---------------------------------------------------------------------------------------------------- D. reduction
def _reduce(scores, P, step, curves):
    import ivf_lib as L
    s = torch.as_tensor(np.asarray(scores, np.float32)).cuda().contiguous()
    b, nc, J1 = s.shape
    ba, auc = guarded((b, nc))
    bn, norm = guarded((b, nc))
    for t in (auc, norm):
        bits(t).fill_(0x7F800000)                                    # +inf: a NaN result is a written result
    L.check(L.lib().ivf_curve_reduce(L.ptr(s), b, nc, curves, P, step, L.ptr(auc), L.ptr(norm), L.stream()))
    torch.cuda.synchronize()
    assert untouched(ba) and untouched(bn)
    assert not bool(torch.isinf(auc).any()) and not bool(torch.isinf(norm).any())
    return auc.cpu().numpy(), norm.cpu().numpy()


def test_reduction_is_exact_on_planted_curves():
    """scores multiples of 2^-8, P a power of two, s_hi - s_lo = 1/2: every fp32 operation is exact"""
    g = np.random.default_rng(3)
    for P, step in ((16, 1), (16, 3), (16, 16), (64, 5), (1, 1)):
        J = -(-P // step)
        s = g.integers(0, 257, (3, 2, J + 1)) / 256.0
        s[:, 0, 0], s[:, 0, J] = 0.75, 0.25                           # deletion: the clip first
        s[:, 1, 0], s[:, 1, J] = 0.25, 0.75
        auc, norm = _reduce(s, P, step, 3)
        ref = CR.auc_ref(s, P, step, 3)
        assert np.array_equal(auc.astype(np.float64), ref["auc"]), (P, step)
        assert np.array_equal(norm.astype(np.float64), ref["auc_norm"]), (P, step)
    # the linear curve: exactly one half
    k = CR.thresholds(16, 3) / 16.0
    auc, norm = _reduce(np.stack([1 - k, k])[None], 16, 3, 3)
    assert auc.tolist() == [[0.5, 0.5]] and norm.tolist() == [[0.5, 0.5]]


def test_reduction_against_fp64_nan_rules_and_batch_independence():
    g = np.random.default_rng(12)
    worst = 0.0
    for P, step, curves, b in ((36, 1, 3, 3), (36, 5, 3, 3), (36, 5, 1, 2), (36, 7, 2, 2), (4096, 1, 3, 2), (4096, 100, 3, 2)):
        J = -(-P // step)
        s = g.random((b, 2 if curves == 3 else 1, J + 1)).astype(np.float32)
        auc, norm = _reduce(s, P, step, curves)
        ref = CR.auc_ref(s, P, step, curves)
        ea, en = np.abs(auc - ref["auc"]), np.abs(norm - ref["auc_norm"])
        worst = max(worst, float((ea / ref["bound_auc"]).max()), float((en / ref["bound_norm"]).max()))
        assert bool((ea <= ref["bound_auc"]).all()), (P, step, curves)
        assert bool((en <= ref["bound_norm"]).all()), (P, step, curves)
        for r in range(b):                                           # rows of a b-clip call == one-clip calls, bit for bit
            a1, n1 = _reduce(s[r:r + 1], P, step, curves)
            assert np.array_equal(a1.view(np.uint32), auc[r:r + 1].view(np.uint32))
            assert np.array_equal(n1.view(np.uint32), norm[r:r + 1].view(np.uint32))
    note(f"curve reduce: worst err / bound {worst:.3f}")
    # any NaN score in a curve makes both of its outputs NaN, and only its
    s = g.random((2, 2, 9)).astype(np.float32)
    clean = _reduce(s, 8, 1, 3)
    for j in (0, 4, 8):
        s2 = s.copy()
        s2[1, 0, j] = np.nan
        auc, norm = _reduce(s2, 8, 1, 3)
        assert np.isnan(auc).tolist() == [[False, False], [True, False]] == np.isnan(norm).tolist(), j
        keep = ~np.isnan(auc)
        assert np.array_equal(auc[keep].view(np.uint32), clean[0][keep].view(np.uint32))
    # s_hi == s_lo: the AUC is a number, the normalised one NaN
    s3 = s.copy()
    s3[0, 1, 8] = s3[0, 1, 0]
    auc, norm = _reduce(s3, 8, 1, 3)
    assert not np.isnan(auc).any() and np.isnan(norm).tolist() == [[False, True], [False, False]]
    # insertion alone takes its ends the other way round
    auc, norm = _reduce(s[:, 1:], 8, 1, 2)
    ref = CR.auc_ref(s[:, 1:], 8, 1, 2)
    assert bool((np.abs(norm - ref["auc_norm"]) <= ref["bound_norm"]).all())


def test_planted_additive_game_orders_the_aucs(clstm):
    """An additive game s(S) = orig - sum_{c in S} w_c with the true marginals as the attribution: the deletion AUC under
    'morf' <= that of each of 8 hash permutations <= that under 'lerf'.  This holds by construction (freezing the
    largest weights first lowers every prefix the most); shap_refs.additive_scores feeds the reduction directly, not the
    network.  Weights and scores are multiples of 2^-12, so every sum of the trapezoid is exact in fp32 and the one division
    by 2P is monotone: the inequalities hold for the device's numbers as they do in exact arithmetic."""
    eng, c = clstm
    grid = (3,) + SR.CHAIN_GRID
    P = 36
    w = np.random.default_rng(8).permutation(200)[:P] / 4096.0                   # distinct, >= 0
    attr = torch.from_numpy(w.astype(np.float32).reshape((1,) + grid)).cuda()
    aucs = {}
    for order in ("morf", "lerf"):
        rk = eng.curve_ranks(attr, grid, SR.CHAIN_SIGMA, order).cpu().numpy().astype(np.int64)
        assert np.array_equal(rk, CR.ranks(w[None], 0 if order == "morf" else 1))
        s = SH.additive_scores(rk, w, 0.75)                                      # [1, 1, P+1]
        auc, _ = eng.curve_reduce(torch.from_numpy(s.astype(np.float32)).cuda(), grid, 1, 1)
        ref = CR.auc_ref(s, P, 1, 1)
        assert abs(float(auc[0, 0]) - ref["auc"][0, 0]) <= ref["bound_auc"][0, 0]
        aucs[order] = float(auc[0, 0])
    hs = SH.additive_scores(SH.ranks(1234, 8, P), w, 0.75)[0][:, None, :]        # 8 "clips" of one curve
    hash_auc, _ = eng.curve_reduce(torch.from_numpy(hs.astype(np.float32)).cuda(), grid, 1, 1)
    hash_auc = hash_auc[:, 0].cpu().numpy()
    assert bool((aucs["morf"] <= hash_auc).all()) and bool((hash_auc <= aucs["lerf"]).all())
    assert aucs["morf"] < aucs["lerf"]
    # the expected random curve of these 8 permutations lies between them as well
    rb = eng.curve_random_baseline(torch.from_numpy(hs[:, 0][None].astype(np.float32)).cuda())
    assert np.array_equal(rb.cpu().numpy().astype(np.float64), CR.random_baseline(hs[:, 0][None]))   # exact: a sum of 8
    ra, _ = eng.curve_reduce(rb, grid, 1, 3)
    assert aucs["morf"] <= float(ra[0, 0]) <= aucs["lerf"]


# ---------------------------------------------------------------------------------------------------- E. fixture
def test_s16_curves_vs_fixture(s16, golden):
    """the 2 x 9 rows of tests/golden/curves.npz within 1e-3 relative, each against its own magnitude (the gate of
    test_gpu_shapley.py::test_s16_scores_vs_fixture); target and ranks exact; the AUCs at steps 1 and 3 against the
    fixture's fp64 within what those gated scores can carry plus the fp32 bound of the reduction"""
    g = golden('curves')
    grid = tuple(int(v) for v in g['grid'])
    assert (grid, float(g['sigma']), int(g['clip'])) == ((2, 2, 2), 0.0, 21)
    x = _s16_x()
    t = int(torch.argmax(s16.forward(x)[0]))
    assert t == int(g['target'])
    attr = torch.from_numpy(g['attr'][None]).cuda()
    for step, rows_of, auc_ref in ((1, np.arange(9), g['auc_step1']), (3, g['step3_rows'], g['auc_step3'])):
        r = s16.faithfulness(x, [t], attr, grid=grid, sigma=0.0, step=step)
        assert np.array_equal(r["curve_ranks"][0].cpu().numpy().astype(np.int64), g['ranks'])
        got = np.stack([r["del_scores"][0].cpu().numpy(), r["ins_scores"][0].cpu().numpy()])
        want = g['scores'][:, rows_of]
        e = rel_err_elem(got, want, FLOOR)
        assert e < 1e-3
        w = np.diff(CR.thresholds(8, step)).astype(np.float64)
        m = np.maximum(np.abs(want.astype(np.float64)), FLOOR)
        slack = 1e-3 * (w * (m[:, :-1] + m[:, 1:])).sum(axis=1) / 16.0 + CR.auc_ref(got[None], 8, step, 3)["bound_auc"][0]
        auc = np.array([float(r["del_auc"][0]), float(r["ins_auc"][0])])
        err = np.abs(auc - auc_ref)
        note(f"curves vs fixture {s16.math} step {step}: rows elementwise rel {e:.2e}, auc err / slack "
             f"{float((err / slack).max()):.3f}")
        assert bool((err <= slack).all())
        assert abs(float(r["score_x"][0]) - float(g['orig'])) < 1e-3 * float(g['orig'])


# ---------------------------------------------------------------------------------------------------- F. surfaces
CURVE_FIELDS = {'ranks', 'deletion', 'insertion', 'del_auc', 'ins_auc', 'del_auc_norm', 'ins_auc_norm'}


def test_faithfulness_video_i3d(smth_model):
    import ivf_recipe as RC
    from faithfulness_videos import FaithfulnessVideo
    x = torch.from_numpy(RC.clip(21))[None]
    prof = np.linspace(1.0, 0.0, 16).astype(np.float32)              # earlier frames matter more
    fv = FaithfulnessVideo(smth_model, step=4)                       # the default grid: 16 frames, 2 x 5 rows
    res, out = fv(x, prof)
    assert set(res) == CURVE_FIELDS | {'score_x'} and tuple(out.shape) == (1, 174)
    assert res['ranks'].tolist() == list(range(16)) and res['deletion'].shape == (5,) == res['insertion'].shape
    assert res['deletion'][0] == res['insertion'][4] and res['deletion'][4] == res['insertion'][0]
    eng = smth_model._engine_for(x.cuda(), min_batch=32)
    pred = int(torch.argmax(out[0]))
    want = eng.faithfulness(x.cuda(), [pred], torch.from_numpy(prof)[None].cuda(), step=4)
    assert np.array_equal(res['deletion'].view(np.uint32), want["del_scores"][0].cpu().numpy().view(np.uint32))
    assert float(res['del_auc']) == float(want["del_auc"][0])
    res3, _ = FaithfulnessVideo(smth_model, grid=(2, 2, 2), sigma=0.0, step=3)(x, np.arange(8.0).reshape(2, 2, 2), index=3)
    assert res3['ranks'].tolist() == [7, 6, 5, 4, 3, 2, 1, 0] and res3['deletion'].shape == (4,)


def test_faithfulness_video_clstm():
    import ivf_lib as L
    import ivf_recipe as RC
    from faithfulness_videos import FaithfulnessVideo
    model = _kth_clstm()
    x = torch.from_numpy(RC.clip(7, 3, 32, 120, 160))[None]
    g = np.random.default_rng(1)
    fv = FaithfulnessVideo(model, grid=(4, 1, 2), step=2, order="lerf", archType="CLSTM")
    res, out = fv(x, g.standard_normal((32, 120, 160)).astype(np.float32), index=2)      # a pixel map, pooled
    assert tuple(out.shape) == (1, 6) and sorted(res['ranks'].tolist()) == list(range(8))
    assert res['deletion'].shape == (5,) and np.isfinite(res['deletion']).all() and np.isfinite(res['ins_auc'])
    assert tuple(fv.last["curve_ranks"].shape) == (1, 8)
    with pytest.raises(L.IvfError):
        FaithfulnessVideo(model, archType="VGG")(x, np.zeros(32, np.float32))
    with pytest.raises(L.IvfError):
        fv(x, np.zeros(32, np.float32))                              # a frame profile cannot rank a spatial grid


def _check_record(rec, methods, grid, step, T):
    P = grid[0] * grid[1] * grid[2]
    J = -(-P // step)
    assert set(rec) == {'true_class', 'pred_class', 'video_id', 'grid', 'step'} | set(methods), sorted(rec)
    assert rec['grid'] == grid and rec['step'] == step
    for m in methods:
        q = rec[m]
        assert set(q) == CURVE_FIELDS, m
        rows = P + 1 if m == 'random' else J + 1                     # the random baseline is at step 1
        assert q['deletion'].shape == (rows,) == q['insertion'].shape and q['deletion'].dtype == np.float32
        if m == 'random':
            assert q['ranks'] is None
            assert np.array_equal(q['deletion'], q['insertion'][::-1])
        else:
            assert sorted(q['ranks'].tolist()) == list(range(P))
            assert q['deletion'][0] == q['insertion'][-1] and q['deletion'][-1] == q['insertion'][0]
        assert all(isinstance(q[k], float) for k in ('del_auc', 'ins_auc', 'del_auc_norm', 'ins_auc_norm'))
        assert np.isfinite(q['del_auc']) and np.isfinite(q['ins_auc'])


def test_smth_driver_with_curves(smth_model, tmp_path, monkeypatch):
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    import ivf_lib as L
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    loader = ivf_find_masks.SyntheticLoader(1, 1, (3, 16, 224, 224), 174, first_id=40)      # one clip: the strips are the cost
    hp = {"batch_size": 1, "gradCamType": "guessed"}
    drv.find_masks(loader, smth_model, hp, 0.01, 0.02, 2, "central", "freeze", classOI=None, doGradCam=True,
                   runTempMask=True, verbose=False, doShapley=True, shapPerms=2, doCurves=True, curveStep=4)
    tm = pickle.load(open(tmp_path / "results" / "allTimeMaskResults_run0_None_.p", "rb"))
    rs = pickle.load(open(tmp_path / "results" / "allCurvesResults_run0_None_.p", "rb"))
    assert len(rs) == len(tm) == 1 and rs[0]['video_id'] == 40
    for rec, trec in zip(rs, tm):
        _check_record(rec, ('time_mask', 'gradcam', 'shap', 'random'), (16, 1, 1), 4, 16)
        assert rec['pred_class'] == trec['pred_class']
        assert rec['time_mask']['ranks'].tolist() == CR.ranks(trec['time_mask'][None], 0)[0].tolist()
    last = ivf_find_masks.find_masks_impl.last_curve_results
    assert len(last) == 1 and all(np.array_equal(a['shap']['deletion'], q['shap']['deletion']) for a, q in zip(last, rs))
    with pytest.raises(L.IvfError):
        drv.find_masks(loader, smth_model, hp, 0.01, 0.02, 2, "central", "reverse", classOI=None, doGradCam=False,
                       runTempMask=True, verbose=False, doCurves=True)


def test_kth_driver_with_curves_on_the_convlstm(tmp_path, monkeypatch):
    import FindMasksComparison_I3D_KTH as drv
    import ivf_find_masks
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    loader = ivf_find_masks.SyntheticLoader(1, 1, (3, 32, 120, 160), 6, first_id=7)
    drv.find_masks(loader, _kth_clstm(), {"batch_size": 1, "gradCamType": "guessed"}, 0.02, 0.04, 2, 1, "central",
                   "freeze", classOI=None, doGradCam=False, runTempMask=True, verbose=False, doCurves=True,
                   curveGrid=(4, 1, 1), curveStep=1)
    rs = pickle.load(open(tmp_path / "results" / "I3d_KTH_allCurvesResults_original_run0.p", "rb"))
    assert len(rs) == 1 and rs[0]['video_id'] == "7"
    _check_record(rs[0], ('time_mask',), (4, 1, 1), 1, 32)           # no Shapley run: no 'random' entry


def test_mask_search_curves_on_a_spatial_grid(clstm):
    """a spatial grid takes the [T,H,W] maps: with only Shapley on, 'shap' and -- the same grid and sigma -- 'random';
    another Shapley sigma and 'random' is left out; methods without a map are left out"""
    import ivf_search
    eng, c = clstm
    x, tg = c['x'].cuda(), _tg(c)
    b = x.shape[0]
    grid = (3,) + SR.CHAIN_GRID
    kw = dict(mask_type="freeze", do_gradcam=False, run_temp_mask=False, do_shapley=True, shap_perms=2, shap_grid=grid,
              do_curves=True, curve_grid=grid, curve_sigma=SR.CHAIN_SIGMA, curve_step=6)
    out = ivf_search.MaskSearch(eng, shap_sigma=SR.CHAIN_SIGMA, **kw).run(x, tg)
    ms = sorted(k[len("curves_"):-len("_deletion")] for k in out if k.startswith("curves_") and k.endswith("_deletion"))
    assert ms == ['random', 'shap']
    assert tuple(out["curves_shap_ranks"].shape) == (b, 36) and tuple(out["curves_shap_deletion"].shape) == (b, 7)
    assert tuple(out["curves_random_deletion"].shape) == (b, 37) and "curves_random_ranks" not in out
    want = eng.curve_ranks(out["shap_map"], grid, SR.CHAIN_SIGMA)
    assert torch.equal(out["curves_shap_ranks"], want)
    out2 = ivf_search.MaskSearch(eng, shap_sigma=2.5, **kw).run(x, tg)
    assert "curves_shap_deletion" in out2 and "curves_random_deletion" not in out2


def test_files_are_byte_identical_with_curves_off(smth_model, tmp_path, monkeypatch):
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    blobs = []
    for sub, extra in (("plain", {}), ("kwargs", dict(doCurves=False, curveGrid=(2, 2, 2), curveSigma=3.0, curveStep=2))):
        d = tmp_path / sub
        d.mkdir()
        monkeypatch.chdir(d)
        loader = ivf_find_masks.SyntheticLoader(1, 1, (3, 16, 224, 224), 174, first_id=40)
        drv.find_masks(loader, smth_model, {"batch_size": 1, "gradCamType": "guessed"}, 0.01, 0.02, 2, "central",
                       "freeze", classOI=None, doGradCam=True, runTempMask=True, verbose=False, **extra)
        files = sorted(q.relative_to(d) for q in d.rglob("*") if q.is_file())
        blobs.append({str(q): (d / q).read_bytes() for q in files})
        assert not any("Curves" in str(q) or "curve" in str(q) for q in files)
    assert blobs[0].keys() == blobs[1].keys()
    assert all(blobs[0][k] == blobs[1][k] for k in blobs[0]), [k for k in blobs[0] if blobs[0][k] != blobs[1][k]]


def test_refusals(clstm):
    import ivf_engine
    import ivf_lib as L
    import ivf_search
    eng, c = clstm
    x, tg = c['x'].cuda(), _tg(c)
    b, T = x.shape[0], x.shape[2]
    prof = torch.rand(b, T, device='cuda')
    for grid in ((T + 1, 1, 1), (0, 1, 1), (3, 33, 4), (3, 3, 0), (3, 4), "abc", (5, 32, 32)):
        with pytest.raises(L.IvfError):
            eng.faithfulness(x, tg, prof, grid=grid)
        with pytest.raises(L.IvfError):
            eng.curve_ranks(prof, grid=grid)
    for kw in (dict(step=0), dict(step=T + 1), dict(step="x"), dict(order="best"), dict(order=2)):
        with pytest.raises(L.IvfError):
            eng.faithfulness(x, tg, prof, **kw)
    with pytest.raises(L.IvfError):
        eng.faithfulness(x, tg, prof, grid=(3, 3, 4))                    # a frame profile on a spatial grid
    with pytest.raises(L.IvfError):
        eng.faithfulness(x, tg, torch.rand(b, T + 1, device='cuda'))     # no accepted shape
    with pytest.raises(L.IvfError):
        eng.faithfulness(x, tg, prof[:1])                                # one attribution for two clips
    with pytest.raises(L.IvfError):
        eng.faithfulness(x, tg[:1], prof)                                # one target for two clips
    rk = eng.curve_ranks(prof)
    with pytest.raises(L.IvfError):
        eng.curve_scores(x, tg, rk, curves=4)
    with pytest.raises(L.IvfError):
        eng.curve_scores(x, tg, rk.int())                                # not int16
    with pytest.raises(L.IvfError):
        eng.curve_scores(x, tg, rk[:, :-1])
    with pytest.raises(L.IvfError):
        eng.curve_reduce(torch.zeros(2, 2, T, device='cuda'))            # T is not J + 1
    with pytest.raises(L.IvfError):
        eng.curve_reduce(torch.zeros(2, 1, T + 1, device='cuda'), curves=3)
    with pytest.raises(L.IvfError):
        eng.curve_random_baseline(torch.zeros(2, T + 1, device='cuda'))
    with pytest.raises(L.IvfError):
        ivf_search.MaskSearch(eng, mask_type="reverse", do_curves=True)
    ivf_search.MaskSearch(eng, mask_type="reverse")                      # off: 'reverse' stays what it was
    # the C entry: null pointers and bad arguments come back as error codes, nothing is written
    lib = L.lib()
    _, _, _, AH, AW = eng._st_axes((1, 1), None)
    sc = torch.full((b, 2, T + 1), -12345.0, device='cuda')
    tgt = torch.as_tensor(tg, dtype=torch.int32, device='cuda')
    fn = lib.ivf_clstm_curve_scores
    ok = [eng._h, L.ptr(x), b, L.ptr(tgt), L.ptr(AH), L.ptr(AW), T, 1, 1, L.ptr(rk), 3, 1, L.ptr(sc), L.stream()]
    for pos, val in ((1, None), (3, None), (4, None), (9, None), (12, None), (2, 0), (6, 0), (6, T + 1), (10, 0), (10, 4),
                     (11, 0), (11, T + 1)):
        a = list(ok)
        a[pos] = val
        assert fn(*a) == -1, (pos, val)
        assert b"curve" in lib.ivf_last_error()
    torch.cuda.synchronize()
    assert bool((sc == -12345.0).all())
    # the TF-style plan has no curve entry and refuses
    tf = ivf_engine.TFCLSTMEngine(5, (1, 8, 30, 40), units=(4,), kernel=(3, 5), stride=2, padding="valid", max_batch=1)
    assert not hasattr(lib, "ivf_tfclstm_curve_scores")
    xt = torch.zeros(1, 1, 8, 30, 40, device='cuda')
    at = torch.zeros(1, 8, device='cuda')
    for call in (lambda: tf.faithfulness(xt, [0], at), lambda: tf.curve_ranks(at), lambda: tf.curve_cells(at),
                 lambda: tf.curve_scores(xt, [0], torch.zeros(1, 8, dtype=torch.int16, device='cuda')),
                 lambda: tf.curve_reduce(torch.zeros(1, 2, 9, device='cuda')),
                 lambda: tf.curve_random_baseline(torch.zeros(1, 2, 9, device='cuda'))):
        with pytest.raises(L.IvfError):
            call()
