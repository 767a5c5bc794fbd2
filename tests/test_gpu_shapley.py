"""Shapley value sampling (csrc/shapley_ops.hip) on the GPU: the rank table against the numpy table,
the staging kernel against ivf_stmask_expand_fwd + ivf_stfreeze_fwd on each row's explicit per-frame S (equality), the
row ends against the clip and ivf_blob_stage's fully frozen row, the score rows against st_perturbed_forward and against
tests/golden/shapley.npz (make_golden_shapley.py: the reference's I3D model under the torch restatement of expand and
per-pixel freeze), the exact invariants of the estimator on the plans (efficiency, the dummy frame 0), the reduction
against the fp64 reference and the derived bounds of tests/shap_refs.py, and the public surfaces.
tests/test_shap_refs_host.py proves the references on the CPU."""
import os
import pickle

import numpy as np
import pytest
import torch

import box_refs as B
import shap_refs as SH
import stmask_refs as SR
from conftest import note, rel_err_elem
from test_gpu_box import FLOOR, _gate
from test_gpu_leaf_kernels import bits, guarded, untouched

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00ABC


def _dev_ranks(rk):
    """a numpy rank table as the int16 device tensor the entries take (uint16 values below 4096)"""
    return torch.from_numpy(np.asarray(rk).astype(np.int16)).cuda().contiguous()


# ---------------------------------------------------------------------------------------------------- A. rank table
@pytest.mark.parametrize("anti", [1, 0])
@pytest.mark.parametrize("grid,first_k,count", [((1, 1, 1), 0, 5), ((3, 3, 4), 0, 6), ((3, 3, 4), 3, 5), ((8, 7, 7), 1000, 7),
                                                ((4, 32, 32), 1, 3)])
def test_rank_table_is_the_numpy_table(grid, first_k, count, anti):
    import ivf_lib as L
    P = grid[0] * grid[1] * grid[2]
    buf, rk = guarded((count, P), dtype=torch.int16, sent=-77)
    rk.fill_(0x7ABC)
    L.check(L.lib().ivf_shap_ranks(1234, anti, first_k, count, *grid, L.ptr(rk), L.stream()))
    torch.cuda.synchronize()
    assert untouched(buf, -77)
    want = SH.ranks(1234, count, P, bool(anti), first_k)
    got = rk.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, want), (grid, first_k, count, anti)
    assert np.array_equal(np.sort(got, axis=1), np.broadcast_to(np.arange(P), (count, P)))
    if grid == (3, 3, 4) and first_k == 0:
        assert (got[1].tolist() == (P - 1 - got[0]).tolist()) == bool(anti)


def test_rank_known_answer_on_the_device():
    import ivf_lib as L
    rk = torch.empty(2, 8, dtype=torch.int16, device='cuda')
    L.check(L.lib().ivf_shap_ranks(1234, 0, 0, 2, 2, 2, 2, L.ptr(rk), L.stream()))
    assert rk.cpu().tolist() == [[1, 0, 7, 2, 4, 3, 6, 5], [7, 3, 0, 6, 4, 5, 1, 2]]


# ---------------------------------------------------------------------------------------------------- B. staging
def _stage(xd, AHd, AWd, dims, rkd, first, count, cpad):
    import ivf_lib as L
    b, C, T, H, W, (gt, gh, gw), n = dims
    buf, out = guarded((count, C, T, H * W) if cpad == 0 else (count, T, H * W, 4))
    bits(out).fill_(NAN_BITS)
    L.check(L.lib().ivf_shap_stage(L.ptr(xd), b, C, T, H, W, L.ptr(AHd), L.ptr(AWd), gt, gh, gw, n, L.ptr(rkd), first, count,
                                   L.ptr(out), cpad, L.stream()))
    torch.cuda.synchronize()
    assert untouched(buf), f"shap_stage out_cpad={cpad}: a sentinel row was written"
    assert not bool(torch.isnan(out).any()), f"shap_stage out_cpad={cpad}: an element was never written"
    return out


def _pair(xd, AHd, AWd, dims, rk, first, count, cpad):
    """the same rows by ivf_stmask_expand_fwd + ivf_stfreeze_fwd on the explicit per-frame S of each row's prefix"""
    import ivf_lib as L
    b, C, T, H, W, grid, n = dims
    gt, gh, gw = grid
    per = n * (gt * gh * gw + 1)
    rows = np.arange(first, first + count)
    S = torch.from_numpy(SH.frame_masks(SH.row_masks(rk, grid, rows % per), T)).cuda().contiguous()     # [count,T,gh,gw]
    xr = xd[torch.from_numpy(rows // per).cuda()].contiguous()
    M = torch.empty(count, T, H, W, device='cuda')
    L.check(L.lib().ivf_stmask_expand_fwd(L.ptr(S), L.ptr(AHd), L.ptr(AWd), L.ptr(M), count, T, gh, gw, H, W, L.stream()))
    out = torch.empty((count, C, T, H * W) if cpad == 0 else (count, T, H * W, 4), device='cuda')
    L.check(L.lib().ivf_stfreeze_fwd(L.ptr(xr), L.ptr(M), L.ptr(out), count, C, T, H * W, cpad, L.stream()))
    torch.cuda.synchronize()
    return out


def _check_windows(C, T, sigma, grid, cpad, windows, H=12, W=20, b=2, n=2, seed=1234, anti=True):
    gt, gh, gw = grid
    P = gt * gh * gw
    per = n * (P + 1)
    dims = (b, C, T, H, W, grid, n)
    xd = B.stage_inputs(b, C, T, H, W, key='shap').cuda()
    AHd, AWd = SR.axis_weights(H, gh, sigma).cuda(), SR.axis_weights(W, gw, sigma).cuda()
    rk = SH.ranks(seed, n, P, anti)
    rkd = _dev_ranks(rk)
    moved = 0
    for first, count in windows:
        assert 0 <= first and first + count <= b * per
        got = _stage(xd, AHd, AWd, dims, rkd, first, count, cpad)
        want = _pair(xd, AHd, AWd, dims, rk, first, count, cpad)
        assert torch.equal(got, want), f"rows [{first}, {first + count}) of {b * per}: not the bits of expand_fwd + stfreeze_fwd"
        if cpad == 4:
            assert torch.equal(bits(got[..., C:]), torch.zeros_like(bits(got[..., C:]))), "pad lane not +0.0"
        src = xd[torch.from_numpy(np.arange(first, first + count) // per).cuda()]
        flat = got if cpad == 0 else got[..., :C].permute(0, 3, 1, 2)
        moved += int((flat != src.reshape(count, C, T, H * W)).any(dim=(1, 2, 3)).sum())
    assert moved > 0, "no staged row differs from its clip: the comparison is vacuous"


# grid (3, 3, 4): P = 36, 37 rows a permutation, n = 2: 74 rows a clip, 148 in all.  Mid-permutation, across the
# permutation boundary (row 37), across the clip boundary (row 74), ending on the last row, the whole list
WINDOWS = [(5, 8), (33, 9), (70, 9), (140, 8), (0, 148)]


@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("sigma", [0.0, 1.5])
@pytest.mark.parametrize("C", [1, 3])
def test_staging_is_expand_plus_freeze_on_the_explicit_mask(C, sigma, cpad):
    """B.  b = 2, T = 5, 12 x 20 (one workgroup with 16 idle threads), grid (3, 3, 4), n = 2"""
    _check_windows(C, 5, sigma, (3, 3, 4), cpad, WINDOWS)


@pytest.mark.parametrize("cpad", [0, 4])
def test_staging_over_several_workgroups(cpad):
    """23 x 27 = 621 pixels: three workgroups per row, the last ragged, rows of pixels that straddle workgroups, a
    second seed without the antithetic pairing; the widest grid row (32 cells: bit 31 of the column word)"""
    _check_windows(3, 6, 1.0, (2, 4, 5), cpad, [(30, 20), (0, 45)], H=23, W=27, n=3, seed=99, anti=False)
    _check_windows(2, 3, 0.7, (3, 2, 32), cpad, [(150, 60), (380, 6)], H=9, W=40, n=1, seed=5)


@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("gt", [1, 4, None])
@pytest.mark.parametrize("T", [17, 40, 16, 32])
def test_staging_on_every_frame_count_path(T, gt, cpad):
    """B at T = 17 and 40 (the frame loop) and T = 16 and 32 (pieces of 16 preloaded frames), with one temporal cell,
    four, and one per frame (gt None = T); spatial grid (1, 2) so that gt = 40 stays small: windows inside the first
    permutation, across the permutation boundary and across the clip boundary"""
    g = (T if gt is None else gt, 1, 2)
    P1 = g[0] * 2 + 1
    _check_windows(3, T, 1.5, g, cpad, [(1, 6), (P1 - 3, 6), (2 * P1 - 4, 8)])


@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("T,grid", [(5, (3, 3, 4)), (16, (16, 1, 1))])
def test_row_ends_and_the_entering_cell(T, grid, cpad):
    """sigma 0: row 0 of a permutation is the clip, bit for bit; row P is ivf_blob_stage's fully frozen row (the blob
    [0, T)); consecutive rows differ only inside the footprint of the entering cell: its frames (and, the freeze being
    a recurrence, the later ones) and its pixel rectangle.  12 x 16 on a (3, 4) grid: the bilinear weights are multiples
    of 1/8, exact in fp32, so the fully set mask expands to exactly 1"""
    import ivf_lib as L
    b, C, H, W, n = 2, 3, 12, 16, 2
    gt, gh, gw = grid
    P = gt * gh * gw
    per = n * (P + 1)
    xd = B.stage_inputs(b, C, T, H, W, key='shap').cuda()
    AHd, AWd = SR.axis_weights(H, gh, 0.0).cuda(), SR.axis_weights(W, gw, 0.0).cuda()
    rk = SH.ranks(1234, n, P)
    got = _stage(xd, AHd, AWd, (b, C, T, H, W, grid, n), _dev_ranks(rk), 0, b * per, cpad)
    nb = L.lib().ivf_blob_count(T, T)
    frozen = torch.empty((b,) + tuple(got.shape[1:]), device='cuda')
    clip = torch.empty_like(frozen)
    zero = torch.zeros(b, T, device='cuda')
    for r in range(b):                                   # candidate nb - 1 of each clip: length T from frame 0
        L.check(L.lib().ivf_blob_stage(L.ptr(xd), b, C, T, H * W, T, 0, r * nb + nb - 1, 1, L.ptr(frozen[r]), cpad, L.stream()))
    L.check(L.lib().ivf_freeze_fwd(L.ptr(xd), L.ptr(zero), L.ptr(clip), b, C, T, H * W, 1, cpad, L.stream()))   # the clip in this layout
    torch.cuda.synchronize()
    assert not torch.equal(frozen, clip)
    # bilinear footprints at sigma 0: A > 0 exactly on the pixels the cell reaches
    AH, AW = SR.axis_weights(H, gh, 0.0).numpy(), SR.axis_weights(W, gw, 0.0).numpy()
    kt = (np.arange(T) * gt) // T
    changed = 0
    for cl in range(b):
        for k in range(n):
            r0 = cl * per + k * (P + 1)
            assert torch.equal(bits(got[r0]), bits(clip[cl])), f"clip {cl} permutation {k}: row 0 is not the clip"
            assert torch.equal(bits(got[r0 + P]), bits(frozen[cl])), f"clip {cl} permutation {k}: row P is not the frozen clip"
            order = np.argsort(rk[k])                    # order[j] = the cell entering between rows j and j + 1
            for j in range(P):
                c = int(order[j])
                ct, ci, cj = c // (gh * gw), (c // gw) % gh, c % gw
                foot = np.outer(AH[:, ci] > 0, AW[:, cj] > 0).reshape(-1)                    # [HW]
                first_frame = int(np.nonzero(kt == ct)[0][0])
                a, z = got[r0 + j], got[r0 + j + 1]
                diff = (a != z)
                diff = diff.any(dim=0) if cpad == 0 else diff.any(dim=2)                      # [T, HW]
                diff = diff.cpu().numpy()
                assert not diff[:first_frame].any(), (cl, k, j, "a frame before the cell changed")
                assert not diff[:, ~foot].any(), (cl, k, j, "a pixel outside the cell's footprint changed")
                changed += int(diff.any())
    assert changed > b * n * P // 2                      # freezing frame 0's cells changes nothing; most others do


# ---------------------------------------------------------------------------------------------------- C. plans
def _s16_x(clips=(21,)):
    import ivf_recipe as RC
    return torch.from_numpy(np.stack([RC.clip(c) for c in clips])).cuda()


@pytest.fixture(scope="module")
def s16():
    """the S16 I3D plan in the default arithmetic"""
    import ivf_engine
    import ivf_recipe as RC
    eng = ivf_engine.I3DEngine(174, (3, 16, 224, 224), max_batch=32, softmax=True)
    eng.load_state_dict(RC.i3d_state_dict(num_classes=174))
    return eng


@pytest.fixture(scope="module")
def clstm():
    """the ConvLSTM plan of clstm_refs case S2 (C 2, T 6, 24 x 32, two layers), as test_gpu_box.py builds it"""
    import ivf_engine
    c = SR.chain_case()
    case = c['case']
    eng = ivf_engine.CLSTMEngine(5, (case.C, case.T, case.H, case.W), max_batch=case.B, hidden=case.hid, layers=case.layers,
                                 kernel=case.k, stride=case.s, softmax=case.softmax, batch_norm=case.batch_norm)
    eng.load_state_dict(c['sd'])
    return eng, c


def _tg(c):
    return [int(v) for v in c['targets']]


def _chain(eng, x, targets, grid, sigma, n, seed, math):
    """shap_scores == st_perturbed_forward of the explicit expanded masks in the same chunk composition (equality); the
    rows of clip 1 of a two-clip call start at another place of their chunk: the other-composition gate"""
    b, T = x.shape[0], x.shape[2]
    P = grid[0] * grid[1] * grid[2]
    per = n * (P + 1)
    Bp = eng.max_batch
    scores = eng.shap_scores(x, targets, n, grid, sigma, seed)
    assert tuple(scores.shape) == (b, n, P + 1)
    rk = SH.ranks(seed, n, P)
    assert np.array_equal(eng.shap_ranks(n, grid, seed).cpu().numpy().astype(np.int64), rk)
    flat = scores.reshape(-1)
    tl = torch.as_tensor(targets, device='cuda').long()
    for first in range(0, b * per, Bp):
        rows = np.arange(first, min(first + Bp, b * per))
        S = torch.from_numpy(SH.frame_masks(SH.row_masks(rk, grid, rows % per), T)).cuda().contiguous()
        clip = torch.from_numpy(rows // per).cuda()
        M = eng.st_expand(S, grid[1:], sigma)
        pr = eng.st_perturbed_forward(x[clip].contiguous(), M)[torch.arange(len(rows), device='cuda'), tl[clip]]
        assert torch.equal(pr, flat[first:first + len(rows)]), f"chunk at row {first}"
    assert len(torch.unique(flat)) > 1
    assert per % Bp != 0
    one = eng.shap_scores(x[1:].contiguous(), list(targets[1:]), n, grid, sigma, seed)
    e = rel_err_elem(scores[1:].cpu().numpy(), one.cpu().numpy(), FLOOR)
    assert e < _gate(math)
    return e


def test_i3d_rows_equal_st_perturbed_forward(s16):
    x = _s16_x((21, 7))
    targets = s16.argmax(s16.forward(x)).tolist()
    e = _chain(s16, x, targets, (2, 2, 2), 0.0, 4, 1234, s16.math)
    note(f"shapley chain I3D {s16.math}: 72 rows bit-equal to st_perturbed_forward; clip 1 at another chunk offset {e:.2e}")


def test_clstm_rows_equal_st_perturbed_forward(clstm):
    eng, c = clstm
    e = _chain(eng, c['x'].cuda(), _tg(c), (3,) + SR.CHAIN_GRID, SR.CHAIN_SIGMA, 1, 1234, "fp32")
    note(f"shapley chain ConvLSTM S2: rows bit-equal to st_perturbed_forward; clip 1 at another chunk offset {e:.2e}")


def _invariants(eng, x, targets, n, sigma, math, what):
    """the default grid (T, 1, 1): the players are the frames.  Frame 0 is a dummy (freezing it changes no input bit, so
    its marginals are differences of the same row at two chunk positions: the other-composition gate, against the
    scores' own magnitude); the cells sum to shap_total within the derived fp32 bounds; shap_total is
    score_x - score(all frozen) within the gate; shap_frames sums to the cells"""
    b, T = x.shape[0], x.shape[2]
    grid = (T, 1, 1)
    r = eng.shapley(x, targets, n_perms=n, sigma=sigma, seed=77)
    assert tuple(r["shap_cells"].shape) == (b,) + grid and tuple(r["shap_scores"].shape) == (b, n, T + 1)
    s = r["shap_scores"].cpu().numpy()
    rk = SH.ranks(77, n, T)
    ref = SH.reduce_ref(s, rk)
    cells = r["shap_cells"].cpu().numpy().reshape(b, T).astype(np.float64)
    se = r["shap_stderr"].cpu().numpy().reshape(b, T).astype(np.float64)
    total = r["shap_total"].cpu().numpy().astype(np.float64)
    gate = _gate(math)
    assert n >= 5                                        # stderr <= max|d - phi| / sqrt(n - 1) <= 2 max|d| / 2
    kk = np.arange(n)
    a, z = s[:, kk, rk[:, 0]], s[:, kk, rk[:, 0] + 1]                              # the two rows around frame 0's entry
    lim = gate * np.maximum(np.maximum(np.abs(a), np.abs(z)), FLOOR).max(axis=1)
    assert bool((np.abs(cells[:, 0]) <= lim).all()), (what, cells[:, 0], lim)
    assert bool((se[:, 0] <= lim).all()), (what, se[:, 0], lim)
    assert bool((np.abs(cells[:, 1:]).max(axis=1) > lim).all()), "no frame matters: the dummy check is vacuous"
    # efficiency
    gap = np.abs(cells.sum(axis=1) - total)
    lim_e = ref["bound_cells"].sum(axis=1) + ref["bound_total"]
    assert bool((gap <= lim_e).all()), (what, gap, lim_e)
    # total against the two end scores computed on their own
    ones = torch.ones(b, T, 1, 1, device='cuda')
    idx = torch.arange(b, device='cuda')
    tl = torch.as_tensor(targets, device='cuda').long()
    frozen = eng.st_perturbed_forward(x, eng.st_expand(ones, (1, 1), sigma))[idx, tl].cpu().numpy().astype(np.float64)
    sx = r["score_x"].cpu().numpy().astype(np.float64)
    lim_t = gate * (np.maximum(np.abs(sx), FLOOR) + np.maximum(np.abs(frozen), FLOOR)) + ref["bound_total"]
    assert bool((np.abs(total - (sx - frozen)) <= lim_t).all()), (what, total, sx - frozen, lim_t)
    # frames
    fr = r["shap_frames"].cpu().numpy().astype(np.float64)
    assert bool((np.abs(fr.sum(axis=1) - cells.sum(axis=1)) <= SH.frames_sum_bound(cells, grid)).all())
    assert np.array_equal(r["shap_frames"].cpu().numpy(), r["shap_cells"].cpu().numpy().reshape(b, T))   # one frame a cell
    note(f"shapley invariants {what}: |phi_0| {float(np.abs(cells[:, 0]).max()):.2e} stderr_0 {float(se[:, 0].max()):.2e} "
         f"(gate {float(lim.min()):.2e}); sum cells - total {float(gap.max()):.2e} (bound {float(lim_e.min()):.2e}); "
         f"total - (score_x - frozen) {float(np.abs(total - (sx - frozen)).max()):.2e}")
    return r


def test_i3d_frame_game_invariants(s16):
    x = _s16_x()
    t = s16.argmax(s16.forward(x)).tolist()
    _invariants(s16, x, t, 6, None, s16.math, f"I3D {s16.math}")


def test_clstm_frame_game_invariants(clstm):
    eng, c = clstm
    _invariants(eng, c['x'].cuda(), _tg(c), 6, None, "fp32", "ConvLSTM S2")


def test_shap_frames_share_a_temporal_cell(clstm):
    """gt < T: a frame's value is its temporal cell's spatial sum divided by the cell's frame count"""
    eng, c = clstm
    x, tg = c['x'].cuda(), _tg(c)
    b, T = x.shape[0], x.shape[2]
    grid = (4,) + SR.CHAIN_GRID                          # T = 6: cells of 2, 1, 2, 1 frames
    r = eng.shapley(x, tg, n_perms=1, grid=grid, sigma=SR.CHAIN_SIGMA, seed=3)
    cells = r["shap_cells"].cpu().numpy().astype(np.float64)
    kt = (np.arange(T) * 4) // T
    nf = np.bincount(kt, minlength=4)
    assert nf.tolist() == [2, 1, 2, 1]
    want = cells.sum(axis=(2, 3))[:, kt] / nf[kt]
    fr = r["shap_frames"].cpu().numpy().astype(np.float64)
    lim = SH.frames_sum_bound(cells, grid)
    assert bool((np.abs(fr - want).max(axis=1) <= lim).all())
    assert bool((np.abs(fr.sum(axis=1) - cells.sum(axis=(1, 2, 3))) <= lim).all())
    S = r["shap_cells"][:, torch.from_numpy(kt).cuda()].contiguous()
    assert torch.equal(r["shap_map"], eng.st_expand(S, grid[1:], SR.CHAIN_SIGMA)) and tuple(r["shap_map"].shape) == (b, T) + tuple(x.shape[3:])
    assert np.isnan(r["shap_stderr"].cpu().numpy()).all() and int(r["shap_count"].min()) == 1     # one permutation


# ---------------------------------------------------------------------------------------------------- D. reduction
def _reduce(scores, rk, grid):
    import ivf_lib as L
    s = torch.as_tensor(np.asarray(scores, np.float32)).cuda().contiguous()
    b, n, P1 = s.shape
    bc, cells = guarded((b,) + grid)
    bs, se = guarded((b,) + grid)
    bn, cnt = guarded((b,) + grid, dtype=torch.int32, sent=-77)
    bt, tot = guarded((b,))
    for t in (cells, se, tot):
        bits(t).fill_(NAN_BITS)
    L.check(L.lib().ivf_shap_reduce(L.ptr(s), L.ptr(_dev_ranks(rk)), b, n, *grid, L.ptr(cells), L.ptr(se), L.ptr(cnt),
                                    L.ptr(tot), L.stream()))
    torch.cuda.synchronize()
    assert untouched(bc) and untouched(bs) and untouched(bn, -77) and untouched(bt)
    P = P1 - 1
    return cells.cpu().numpy().reshape(b, P), se.cpu().numpy().reshape(b, P), cnt.cpu().numpy().reshape(b, P), tot.cpu().numpy()


def _check_reduce(scores, rk, grid, what):
    s32 = np.asarray(scores, np.float32)
    cells, se, cnt, tot = _reduce(s32, rk, grid)
    ref = SH.reduce_ref(s32, rk)
    assert np.array_equal(cnt, ref["count"]), f"{what}: counts differ"
    assert np.array_equal(np.isnan(cells), ref["count"] == 0), f"{what}: NaN cells exactly where nothing is counted"
    assert np.array_equal(np.isnan(se), ref["count"] < 2), f"{what}: NaN stderr exactly where fewer than two terms"
    assert np.array_equal(np.isnan(tot), ref["nall"] == 0)
    worst = {}
    for name, got, want, bound, ok in (("cells", cells, ref["cells"], ref["bound_cells"], ref["count"] > 0),
                                       ("stderr", se, ref["stderr"], ref["bound_stderr"], ref["count"] >= 2),
                                       ("total", tot, ref["total"], ref["bound_total"], ref["nall"] > 0)):
        err = np.abs(got.astype(np.float64) - want)
        worst[name] = float((err[ok] / np.maximum(bound[ok], 1e-300)).max()) if ok.any() else 0.0
        assert bool((err[ok] <= bound[ok]).all()), f"{what}: {name} off by {float((err[ok] - bound[ok]).max()):.3e} beyond the bound"
    print(f"[shap reduce] {what}: worst err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return cells, se, cnt, tot, ref


def test_reduction_recovers_a_planted_additive_game():
    g = np.random.default_rng(4)
    for grid, n in (((2, 2, 2), 1), ((2, 2, 2), 7), ((4, 3, 3), 64), ((1, 1, 1), 3)):
        P = grid[0] * grid[1] * grid[2]
        w = g.integers(-40, 120, P) / 4096.0                         # multiples of 2^-12: the scores are exact in fp32
        rk = SH.ranks(1234, n, P)
        s = SH.additive_scores(rk, w, 0.75)
        assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
        cells, se, cnt, tot, ref = _check_reduce(s, rk, grid, f"additive game {grid} n {n}")
        assert np.array_equal(ref["cells"][0], w) and ref["total"][0] == w.sum()
        assert bool((np.abs(cells[0] - w) <= ref["bound_cells"][0]).all())
        assert abs(float(tot[0]) - w.sum()) <= ref["bound_total"][0]
        if n >= 2:
            assert bool((se[0] <= ref["bound_stderr"][0]).all())      # fp64 stderr is 0
    # weights that are no fp32 numbers: the marginals of a cell differ by roundings, stderr stays within its bound of 0
    rk = SH.ranks(5, 33, 10)
    _check_reduce(SH.additive_scores(rk, np.full(10, 0.1), 3.3), rk, (10, 1, 1), "additive game, w = 0.1")


def test_reduction_against_fp64_with_nan_scores():
    g = np.random.default_rng(11)
    grid, n, b = (4, 3, 3), 9, 3
    P = 36
    rk = SH.ranks(1234, n, P)
    s = g.random((b, n, P + 1)).astype(np.float32)
    cells, se, cnt, tot, _ = _check_reduce(s, rk, grid, "random scores")
    assert int(cnt.min()) == n
    # rows of a b-clip call == one-clip calls, bit for bit
    for r in range(b):
        c1, s1, n1, t1 = _reduce(s[r:r + 1], rk, grid)
        assert np.array_equal(c1.view(np.uint32), cells[r:r + 1].view(np.uint32))
        assert np.array_equal(s1.view(np.uint32), se[r:r + 1].view(np.uint32)) and np.array_equal(n1, cnt[r:r + 1])
        assert np.array_equal(t1.view(np.uint32), tot[r:r + 1].view(np.uint32))
    # a NaN at prefix 5 of permutation 2 removes exactly the two marginals that touch it
    s2 = s.copy()
    s2[1, 2, 5] = np.nan
    s2[2, :, :] = np.nan                                             # a clip with nothing left
    s2[0, 4, 0] = np.nan                                             # an end score: the permutation leaves total
    c2, e2, n2, t2, ref2 = _check_reduce(s2, rk, grid, "NaN scores")
    hit = (rk[2] == 4) | (rk[2] == 5)
    assert np.array_equal(cnt[1] - n2[1], hit.astype(cnt.dtype))
    assert np.array_equal(c2[1][~hit].view(np.uint32), cells[1][~hit].view(np.uint32))
    assert np.isnan(c2[2]).all() and not n2[2].any() and np.isnan(t2[2])
    assert ref2["nall"].tolist() == [n - 1, n, 0]
    # an infinite end score is not NaN -- its marginal is formed and counted -- but the permutation is not in total
    s5 = s[:1].copy()
    s5[0, 6, P] = np.inf
    _, _, n5, t5 = _reduce(s5, rk, grid)
    ref5 = SH.reduce_ref(s5, rk)
    assert int(n5.min()) == n and ref5["nall"].tolist() == [n - 1]
    assert abs(float(t5[0]) - ref5["total"][0]) <= ref5["bound_total"][0]
    assert np.array_equal(cnt[0] - n2[0], (rk[4] == 0).astype(cnt.dtype))
    # two permutations, one hit: a count of 1 has a value and no stderr
    s3 = s[:1, :2].copy()
    s3[0, 0, 7] = np.nan
    c3, e3, n3, _, _ = _check_reduce(s3, rk[:2], grid, "two permutations, one NaN")
    assert sorted(set(n3.reshape(-1).tolist())) == [1, 2] and np.array_equal(np.isnan(e3), n3 < 2)
    # the largest table
    rk4 = SH.ranks(77, 3, 4096, antithetic=False)
    _check_reduce(g.random((1, 3, 4097)).astype(np.float32), rk4, (4, 32, 32), "4096 players")


def test_reduce_skips_ranks_outside_the_table():
    """the table is the caller's: a rank >= P forms no term and reads nothing"""
    grid, n = (2, 2, 2), 3
    rk = SH.ranks(9, n, 8)
    bad = rk.copy()
    bad[1, 3] = 8
    bad[2, 3] = 4095
    s = np.random.default_rng(2).random((1, n, 9)).astype(np.float32)
    cells, se, cnt, tot = _reduce(s, bad, grid)
    assert cnt[0].tolist() == [3, 3, 3, 1, 3, 3, 3, 3]
    assert cells[0, 3] == np.float32(s[0, 0, rk[0, 3]] - s[0, 0, rk[0, 3] + 1]) and np.isnan(se[0, 3])


# ---------------------------------------------------------------------------------------------------- E. fixture
def test_s16_scores_vs_fixture(s16, golden):
    """the 36 rows of tests/golden/shapley.npz within 1e-3 relative, each against its own magnitude (the gate of
    test_gpu_rise.py on rise.npz); target bit-exact; the cells against the fixture's fp64 estimator within the error
    those gated scores can carry (shap_refs.gated_cells_slack) plus the fp32 bound of the reduction"""
    g = golden('shapley')
    grid, n, seed = tuple(int(v) for v in g['grid']), int(g['n']), int(g['seed'])
    assert (grid, n, seed, int(g['antithetic']), float(g['sigma']), int(g['clip'])) == ((2, 2, 2), 4, 1234, 1, 0.0, 21)
    rk = SH.ranks(seed, n, 8)
    assert np.array_equal(g['ranks'], rk)
    x = _s16_x()
    t = int(torch.argmax(s16.forward(x)[0]))
    assert t == int(g['target'])                                    # integer output: bit-exact
    r = s16.shapley(x, [t], n_perms=n, grid=grid, sigma=0.0, seed=seed, antithetic=True)
    got = r["shap_scores"][0].cpu().numpy()
    e = rel_err_elem(got, g['scores'], FLOOR)
    eo = abs(float(r["score_x"][0]) - float(g['orig']))
    assert e < 1e-3
    assert eo < 1e-3 * float(g['orig'])
    assert np.array_equal(r["shap_count"][0].cpu().numpy(), g['count'])
    ref = SH.reduce_ref(got[None], rk)
    slack = SH.gated_cells_slack(g['scores'][None], rk, 1e-3, FLOOR)[0] + ref["bound_cells"][0]
    err = np.abs(r["shap_cells"][0].cpu().numpy().reshape(-1).astype(np.float64) - g['cells'].reshape(-1))
    note(f"shapley scores vs fixture {s16.math}: {n * 9} rows, elementwise rel {e:.2e}, orig {eo:.2e} abs, "
         f"cells err / slack {float((err / slack).max()):.3f}")
    assert bool((err <= slack).all())
    assert abs(float(r["shap_total"][0]) - float(g['total'])) <= \
        1e-3 * float(np.maximum(np.abs(g['scores'][:, [0, 8]]), FLOOR).sum()) / n + ref["bound_total"][0]
    assert tuple(r["shap_map"].shape) == (1, 16, 224, 224) and tuple(r["shap_frames"].shape) == (1, 16)


# ---------------------------------------------------------------------------------------------------- F. surfaces
SHAP_OUT = {"shap_scores", "shap_cells", "shap_stderr", "shap_count", "shap_total", "score_x", "shap_map", "shap_frames"}


def test_engine_shapley_outputs_and_determinism(clstm):
    """shapley() on the small ConvLSTM plan: the pieces agree with the entries they are made of; two runs give the same
    bits; b = 1 against b = 2 within the other-composition gate; b beyond max_batch"""
    eng, c = clstm
    x, tg = c['x'].cuda(), _tg(c)
    b, C, T, H, W = x.shape
    grid, sigma, n = (3,) + SR.CHAIN_GRID, SR.CHAIN_SIGMA, 2
    r = eng.shapley(x, tg, n_perms=n, grid=grid, sigma=sigma, seed=9)
    assert set(r) == SHAP_OUT
    assert torch.equal(r["shap_scores"], eng.shap_scores(x, tg, n, grid, sigma, 9))
    idx = torch.arange(b, device='cuda')
    assert torch.equal(r["score_x"], eng.forward(x)[idx, torch.as_tensor(tg, device='cuda')])
    cells, se, cnt, tot = _reduce(r["shap_scores"].cpu().numpy(), SH.ranks(9, n, 36), grid)
    assert np.array_equal(cells.view(np.uint32), r["shap_cells"].cpu().numpy().reshape(b, -1).view(np.uint32))
    assert np.array_equal(se.view(np.uint32), r["shap_stderr"].cpu().numpy().reshape(b, -1).view(np.uint32))
    assert np.array_equal(cnt, r["shap_count"].cpu().numpy().reshape(b, -1)) and r["shap_count"].dtype == torch.int32
    assert np.array_equal(tot.view(np.uint32), r["shap_total"].cpu().numpy().view(np.uint32))
    again = eng.shapley(x, tg, n_perms=n, grid=grid, sigma=sigma, seed=9)
    for k in SHAP_OUT:
        assert torch.equal(bits(again[k]) if again[k].is_floating_point() else again[k],
                           bits(r[k]) if r[k].is_floating_point() else r[k]), k
    one = eng.shapley(x[:1].contiguous(), tg[:1], n_perms=n, grid=grid, sigma=sigma, seed=9)
    assert rel_err_elem(one["shap_scores"].cpu().numpy(), r["shap_scores"][:1].cpu().numpy(), FLOOR) < _gate("fp32")
    # antithetic off and another seed are other games' samples
    assert not torch.equal(eng.shap_ranks(n, grid, 9, antithetic=False), eng.shap_ranks(n, grid, 9))
    assert not torch.equal(eng.shap_ranks(n, grid, 10), eng.shap_ranks(n, grid, 9))
    # b beyond max_batch: the same clips twice give the same rows twice
    x4 = torch.cat([x, x])
    r4 = eng.shapley(x4, tg + tg, n_perms=n, grid=grid, sigma=sigma, seed=9)
    assert tuple(r4["shap_scores"].shape) == (2 * b, n, 37) and tuple(r4["shap_cells"].shape) == (2 * b,) + grid
    for half in (r4["shap_scores"][:b], r4["shap_scores"][b:]):
        assert rel_err_elem(half.cpu().numpy(), r["shap_scores"].cpu().numpy(), FLOOR) < _gate("fp32")
    # the default grid: the frames
    assert tuple(eng.shap_ranks(4).shape) == (4, T)


@pytest.fixture(scope="module")
def smth_model():
    import ivf_recipe as RC
    from models import I3D_doubled
    m = I3D_doubled.Model(174, last_stride=1, stride_mod_layers="", softMax=1)
    m.load_state_dict(RC.to_torch(RC.i3d_state_dict(num_classes=174)))
    return m.cuda().eval()


def _kth_clstm():
    import ivf_recipe as RC
    from models import CLSTM_4
    m = CLSTM_4.Model(num_classes=6, nb_lstm_units=4, channels=3, conv_kernel_size=(5, 5), lstm_layers=2, step=32,
                      image_size=(160, 120), conv_stride=2, effective_step=[7, 15, 23, 31])
    m.load_state_dict(RC.to_torch(RC.clstm_state_dict(channels=3, tag='clstm3')))
    return m.cuda().eval()


def test_shapley_video_i3d(smth_model):
    import ivf_recipe as RC
    from shapley_videos import ShapleyVideo
    x = torch.from_numpy(RC.clip(21))[None]
    sv = ShapleyVideo(smth_model, n_perms=2, seed=3)                 # the default grid: 16 frames, 34 rows
    m, out = sv(x)
    assert m.shape == (16, 224, 224) and m.dtype == np.float32 and tuple(out.shape) == (1, 174)
    assert np.isfinite(m).all() and m.any()
    assert tuple(sv.last["shap_cells"].shape) == (1, 16, 1, 1) and tuple(sv.last["shap_scores"].shape) == (1, 2, 17)
    eng = smth_model._engine_for(x.cuda(), min_batch=32)
    pred = int(torch.argmax(out[0]))
    want = eng.shapley(x.cuda(), [pred], n_perms=2, seed=3)["shap_map"][0].cpu().numpy()
    assert np.array_equal(m.view(np.uint32), want.view(np.uint32))           # index None = the argmax; two runs, same bits
    m3, _ = ShapleyVideo(smth_model, n_perms=2, grid=(2, 2, 2), seed=3)(x, index=3)
    assert m3.shape == (16, 224, 224) and not np.array_equal(m3.view(np.uint32), m.view(np.uint32))
    assert set(sv.last) == SHAP_OUT


def test_shapley_video_clstm():
    import ivf_lib as L
    import ivf_recipe as RC
    from shapley_videos import ShapleyVideo
    model = _kth_clstm()
    x = torch.from_numpy(RC.clip(7, 3, 32, 120, 160))[None]
    sv = ShapleyVideo(model, n_perms=2, grid=(4, 1, 2), seed=1, antithetic=False, archType="CLSTM")
    m, out = sv(x, index=2)
    assert m.shape == (32, 120, 160) and m.dtype == np.float32 and tuple(out.shape) == (1, 6)
    assert tuple(sv.last["shap_cells"].shape) == (1, 4, 1, 2) and tuple(sv.last["shap_scores"].shape) == (1, 2, 9)
    with pytest.raises(L.IvfError):
        ShapleyVideo(model, archType="VGG")(x)


SHAP_KEYS = {'true_class', 'pred_class', 'video_id', 'ShapHeatMap', 'ShapCells', 'ShapStderr', 'ShapFrames', 'shap_total',
             'n_perms', 'seed'}


def test_smth_driver_with_shapley(smth_model, tmp_path, monkeypatch):
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    import ivf_lib as L
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    loader = ivf_find_masks.SyntheticLoader(2, 2, (3, 16, 224, 224), 174, first_id=40)
    hp = {"batch_size": 2, "gradCamType": "guessed"}
    drv.find_masks(loader, smth_model, hp, 0.01, 0.02, 2, "central", "freeze", classOI=None, doGradCam=False,
                   runTempMask=True, verbose=False, doShapley=True, shapPerms=2, shapGrid=(2, 2, 2), shapSeed=5)
    tm = pickle.load(open(tmp_path / "results" / "allTimeMaskResults_run0_None_.p", "rb"))
    rs = pickle.load(open(tmp_path / "results" / "allShapleyResults_run0_None_.p", "rb"))
    assert len(rs) == len(tm) == 2
    for rec, trec in zip(rs, tm):
        assert set(rec) == SHAP_KEYS
        assert rec['ShapHeatMap'].shape == (16, 224, 224) and rec['ShapHeatMap'].dtype == np.float32
        assert rec['ShapCells'].shape == (2, 2, 2) and rec['ShapStderr'].shape == (2, 2, 2) and rec['ShapFrames'].shape == (16,)
        assert rec['pred_class'] == trec['pred_class'] and (rec['n_perms'], rec['seed']) == (2, 5)
        assert isinstance(rec['shap_total'], float) and np.isfinite(rec['ShapCells']).all()
        assert abs(float(rec['ShapFrames'].astype(np.float64).sum()) - float(rec['ShapCells'].astype(np.float64).sum())) \
            <= SH.frames_sum_bound(rec['ShapCells'][None], (2, 2, 2))[0]
    assert rs[0]['video_id'] == 40
    last = ivf_find_masks.find_masks_impl.last_shap_results
    assert len(last) == 2 and all(np.array_equal(a['ShapHeatMap'], q['ShapHeatMap']) for a, q in zip(last, rs))
    assert pickle.load(open(tmp_path / "results" / "allGradCamResults_run0_None_.p", "rb")) == []
    assert not (tmp_path / "results" / "allRiseResults_run0_None_.p").exists()
    strips = [q for q in (tmp_path / "cam_saved_images").rglob("shapley/*.png")]
    assert any(q.name == "casefreeze40_15.png" for q in strips) and any(q.name == "casereverse41_0.png" for q in strips)
    assert all(os.path.isdir(os.path.join(os.path.dirname(os.path.dirname(str(q))), "combined")) for q in strips)
    with pytest.raises(L.IvfError):
        drv.find_masks(loader, smth_model, hp, 0.01, 0.02, 2, "central", "reverse", classOI=None, doGradCam=False,
                       runTempMask=True, verbose=False, doShapley=True, shapPerms=2, shapGrid=(2, 2, 2))


def test_kth_driver_with_shapley_on_the_convlstm(tmp_path, monkeypatch):
    import FindMasksComparison_I3D_KTH as drv
    import ivf_find_masks
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    loader = ivf_find_masks.SyntheticLoader(1, 1, (3, 32, 120, 160), 6, first_id=7)      # one clip: the strips are the cost
    drv.find_masks(loader, _kth_clstm(), {"batch_size": 1, "gradCamType": "guessed"}, 0.02, 0.04, 2, 1, "central",
                   "freeze", classOI=None, doGradCam=False, runTempMask=True, verbose=False, doShapley=True, shapPerms=2,
                   shapGrid=(4, 1, 2), shapSeed=2)
    tm = pickle.load(open(tmp_path / "results" / "I3d_KTH_allTimeMaskResults_original_run0.p", "rb"))
    rs = pickle.load(open(tmp_path / "results" / "I3d_KTH_allShapleyResults_original_run0.p", "rb"))
    assert len(rs) == len(tm) == 1 and all(set(r_) == SHAP_KEYS for r_ in rs)
    assert all(r_['ShapHeatMap'].shape == (32, 120, 160) and r_['ShapCells'].shape == (4, 1, 2) for r_ in rs)
    assert rs[0]['video_id'] == "7"
    assert len(list((tmp_path / "cam_saved_images").rglob("shapley/mygif.gif"))) == 1


def test_files_are_byte_identical_with_shapley_off(smth_model, tmp_path, monkeypatch):
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    blobs = []
    for sub, extra in (("plain", {}), ("kwargs", dict(doShapley=False, shapPerms=7, shapGrid=(2, 2, 2), shapSigma=3.0,
                                                     shapSeed=9))):
        d = tmp_path / sub
        d.mkdir()
        monkeypatch.chdir(d)
        loader = ivf_find_masks.SyntheticLoader(1, 1, (3, 16, 224, 224), 174, first_id=40)
        drv.find_masks(loader, smth_model, {"batch_size": 1, "gradCamType": "guessed"}, 0.01, 0.02, 2, "central",
                       "freeze", classOI=None, doGradCam=True, runTempMask=True, verbose=False, **extra)
        files = sorted(q.relative_to(d) for q in d.rglob("*") if q.is_file())
        blobs.append({str(q): (d / q).read_bytes() for q in files})
        assert not any("Shap" in str(q) or "shap" in str(q) for q in files)
    assert blobs[0].keys() == blobs[1].keys()
    assert all(blobs[0][k] == blobs[1][k] for k in blobs[0]), [k for k in blobs[0] if blobs[0][k] != blobs[1][k]]


def test_refusals(clstm):
    import ivf_engine
    import ivf_lib as L
    import ivf_search
    eng, c = clstm
    x, tg = c['x'].cuda(), _tg(c)
    T = x.shape[2]
    for grid in ((T + 1, 3, 4), (0, 3, 4), (3, 33, 4), (3, 3, 0), (3, 4), "abc", (5, 32, 32)):
        with pytest.raises(L.IvfError):
            eng.shapley(x, tg, n_perms=2, grid=grid)
        with pytest.raises(L.IvfError):
            eng.shap_ranks(2, grid=grid)
    with pytest.raises(L.IvfError):
        eng.shapley(x, tg, n_perms=0, grid=(3, 3, 4))
    with pytest.raises(L.IvfError):
        eng.shapley(x, tg, n_perms=2, grid=(3, 3, 4), seed=-1)
    with pytest.raises(L.IvfError):
        eng.shapley(x, tg[:1], n_perms=2, grid=(3, 3, 4))                # one target for two clips
    with pytest.raises(L.IvfError):
        eng.shap_reduce(torch.zeros(2, 2, 30, device='cuda'), (3, 3, 4))  # 30 is not P + 1
    with pytest.raises(L.IvfError):
        ivf_search.MaskSearch(eng, mask_type="reverse", do_shapley=True)
    ivf_search.MaskSearch(eng, mask_type="reverse")                     # off: 'reverse' stays what it was
    # the C entry: null pointers and a bad grid come back as error codes, nothing is written
    lib = L.lib()
    _, _, _, AH, AW = eng._st_axes((3, 4), 1.0)
    sc = torch.full((2, 2, 37), -12345.0, device='cuda')
    tgt = torch.as_tensor(tg, dtype=torch.int32, device='cuda')
    rk = eng.shap_ranks(2, (3, 3, 4), 1)
    fn = lib.ivf_clstm_shap_scores
    assert fn(eng._h, None, 2, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 3, 4, 2, L.ptr(rk), L.ptr(sc), L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 2, L.ptr(tgt), None, L.ptr(AW), 3, 3, 4, 2, L.ptr(rk), L.ptr(sc), L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 2, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 3, 4, 2, None, L.ptr(sc), L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 2, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 3, 4, 2, L.ptr(rk), None, L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 0, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 3, 4, 2, L.ptr(rk), L.ptr(sc), L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 2, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 3, 4, 0, L.ptr(rk), L.ptr(sc), L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 2, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 0, 3, 4, 2, L.ptr(rk), L.ptr(sc), L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 2, L.ptr(tgt), L.ptr(AH), L.ptr(AW), T + 1, 3, 4, 2, L.ptr(rk), L.ptr(sc), L.stream()) == -1
    assert b"shap" in lib.ivf_last_error()
    torch.cuda.synchronize()
    assert bool((sc == -12345.0).all())
    # the TF-style plan has no Shapley entry and refuses
    tf = ivf_engine.TFCLSTMEngine(5, (1, 8, 30, 40), units=(4,), kernel=(3, 5), stride=2, padding="valid", max_batch=1)
    assert not hasattr(lib, "ivf_tfclstm_shap_scores")
    xt = torch.zeros(1, 1, 8, 30, 40, device='cuda')
    for call in (lambda: tf.shapley(xt, [0], n_perms=2, grid=(2, 2, 2)), lambda: tf.shap_scores(xt, [0], 2, (2, 2, 2)),
                 lambda: tf.shap_ranks(2, grid=(2, 2, 2)), lambda: tf.shap_reduce(torch.zeros(1, 2, 9, device='cuda'), (2, 2, 2))):
        with pytest.raises(L.IvfError):
            call()
