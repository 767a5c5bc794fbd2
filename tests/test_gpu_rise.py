"""RISE random-mask saliency (csrc/rise_ops.hip) on the GPU: the mask bits against the numpy hash, the
staging kernel against ivf_stmask_expand_fwd + ivf_stfreeze_fwd on the explicit per-frame S (equality), the degenerate
1 x 1 x 1 grid against the clip and ivf_blob_stage's fully frozen row, the score rows against st_perturbed_forward and
against tests/golden/rise.npz (make_golden_rise.py: the reference's I3D model under the torch restatement of expand and
per-pixel freeze), the reduction against the fp64 reference of tests/rise_refs.py, and the public surfaces.
tests/test_rise_refs_host.py proves the references on the CPU."""
import os
import pickle

import numpy as np
import pytest
import torch

import box_refs as B
import rise_refs as RR
import stmask_refs as SR
from conftest import note, rel_err_elem
from test_gpu_box import FLOOR, _gate
from test_gpu_leaf_kernels import bits, guarded, untouched

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00ABC


# ---------------------------------------------------------------------------------------------------- A. mask bits
@pytest.mark.parametrize("p", [0.5, 0.25])
@pytest.mark.parametrize("seed", [1234, 0xDEADBEEF])
def test_mask_bits_are_the_numpy_hash(seed, p):
    import ivf_lib as L
    for grid, first_k, count in (((3, 3, 4), 0, 16), ((3, 3, 4), 5, 11), ((8, 7, 7), 1000, 70), ((1, 1, 1), 0, 64),
                                 ((64, 32, 32), 3, 2)):
        buf, S = guarded((count,) + grid)
        bits(S).fill_(NAN_BITS)
        L.check(L.lib().ivf_rise_masks(seed, RR.thresh(p), first_k, count, *grid, L.ptr(S), L.stream()))
        torch.cuda.synchronize()
        assert untouched(buf)
        want = RR.masks(seed, p, count, grid, first_k)
        assert np.array_equal(S.cpu().numpy(), want), (grid, first_k, count)
        assert 0.0 < want.mean() < 1.0
    if seed == 1234 and p == 0.5:
        row = RR.masks(seed, p, 1, (1, 3, 4))[0].reshape(-1)
        assert "".join("1" if v else "0" for v in row) == "110111001010"


# ---------------------------------------------------------------------------------------------------- B. staging
def _stage(xd, AHd, AWd, dims, first, count, cpad):
    import ivf_lib as L
    b, C, T, H, W, (gt, gh, gw), n, seed, p = dims
    buf, out = guarded((count, C, T, H * W) if cpad == 0 else (count, T, H * W, 4))
    bits(out).fill_(NAN_BITS)
    L.check(L.lib().ivf_rise_stage(L.ptr(xd), b, C, T, H, W, L.ptr(AHd), L.ptr(AWd), gt, gh, gw, n, seed, RR.thresh(p),
                                   first, count, L.ptr(out), cpad, L.stream()))
    torch.cuda.synchronize()
    assert untouched(buf), f"rise_stage out_cpad={cpad}: a sentinel row was written"
    assert not bool(torch.isnan(out).any()), f"rise_stage out_cpad={cpad}: an element was never written"
    return out


def _pair(xd, AHd, AWd, dims, S_all, first, count, cpad):
    """the same rows by ivf_stmask_expand_fwd + ivf_stfreeze_fwd on the explicit per-frame S of each row's mask"""
    import ivf_lib as L
    b, C, T, H, W, (gt, gh, gw), n, seed, p = dims
    rows = np.arange(first, first + count)
    S = S_all[torch.from_numpy(rows % n).cuda()].contiguous()                    # [count,T,gh,gw]
    xr = xd[torch.from_numpy(rows // n).cuda()].contiguous()
    M = torch.empty(count, T, H, W, device='cuda')
    L.check(L.lib().ivf_stmask_expand_fwd(L.ptr(S), L.ptr(AHd), L.ptr(AWd), L.ptr(M), count, T, gh, gw, H, W, L.stream()))
    out = torch.empty((count, C, T, H * W) if cpad == 0 else (count, T, H * W, 4), device='cuda')
    L.check(L.lib().ivf_stfreeze_fwd(L.ptr(xr), L.ptr(M), L.ptr(out), count, C, T, H * W, cpad, L.stream()))
    torch.cuda.synchronize()
    return out


def _check_windows(C, T, sigma, grid, cpad, windows, H=12, W=20, b=2, n=16, seed=1234, p=0.5):
    gt, gh, gw = grid
    dims = (b, C, T, H, W, grid, n, seed, p)
    xd = B.stage_inputs(b, C, T, H, W, key='rise').cuda()
    AHd, AWd = SR.axis_weights(H, gh, sigma).cuda(), SR.axis_weights(W, gw, sigma).cuda()
    S_all = torch.from_numpy(RR.frame_masks(RR.masks(seed, p, n, grid), T)).cuda()
    moved = 0
    for first, count in windows:
        assert 0 <= first and first + count <= b * n
        got = _stage(xd, AHd, AWd, dims, first, count, cpad)
        want = _pair(xd, AHd, AWd, dims, S_all, first, count, cpad)
        assert torch.equal(got, want), f"rows [{first}, {first + count}) of {b * n}: not the bits of expand_fwd + stfreeze_fwd"
        if cpad == 4:
            assert torch.equal(bits(got[..., C:]), torch.zeros_like(bits(got[..., C:]))), "pad lane not +0.0"
        src = xd[torch.from_numpy(np.arange(first, first + count) // n).cuda()]
        flat = got if cpad == 0 else got[..., :C].permute(0, 3, 1, 2)
        moved += int((flat != src.reshape(count, C, T, H * W)).any(dim=(1, 2, 3)).sum())
    assert moved > 0, "no staged row differs from its clip: the comparison is vacuous"


# windows of the 32 rows of two clips: mid-clip, across the clip boundary, ending on the last row, the whole list
WINDOWS = [(5, 8), (12, 8), (24, 8), (0, 32)]


@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("sigma", [0.0, 1.5])
@pytest.mark.parametrize("C", [1, 3])
def test_staging_is_expand_plus_freeze_on_the_explicit_mask(C, sigma, cpad):
    """B.  b = 2, T = 5, 12 x 20 (one workgroup with 16 idle threads), grid (3, 3, 4), n = 16"""
    _check_windows(C, 5, sigma, (3, 3, 4), cpad, WINDOWS)


@pytest.mark.parametrize("cpad", [0, 4])
def test_staging_over_several_workgroups(cpad):
    """23 x 27 = 621 pixels: three workgroups per row, the last ragged, rows of pixels that straddle workgroups; a
    second seed and p = 0.25; the widest grid row (32 cells: bit 31 of the column word)"""
    _check_windows(3, 6, 1.0, (2, 4, 5), cpad, [(3, 9), (0, 14)], H=23, W=27, n=7, seed=99, p=0.25)
    _check_windows(2, 3, 0.7, (3, 2, 32), cpad, [(1, 5)], H=9, W=40, n=3, seed=5)


@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("gt", [1, 4, None])
@pytest.mark.parametrize("T", [17, 40, 16, 32])
def test_staging_on_every_frame_count_path(T, gt, cpad):
    """B at T = 17 and 40 (the frame loop) and T = 16 and 32 (pieces of 16 preloaded frames), with one temporal cell,
    four, and one per frame (gt None = T)"""
    _check_windows(3, T, 1.5, (T if gt is None else gt, 3, 4), cpad, [(9, 12), (20, 12)])


@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("T", [5, 16])
def test_1x1x1_grid_rows_are_the_clip_or_the_frozen_clip(T, cpad):
    """grid (1, 1, 1), sigma 0: A is all ones and M = the mask's one bit on every frame -- a row is its clip, bit for bit,
    or ivf_blob_stage's fully frozen row (the blob [0, T))"""
    import ivf_lib as L
    b, C, H, W, n, seed, p = 2, 3, 12, 20, 16, 1234, 0.5
    xd = B.stage_inputs(b, C, T, H, W, key='rise').cuda()
    AHd, AWd = SR.axis_weights(H, 1, 0.0).cuda(), SR.axis_weights(W, 1, 0.0).cuda()
    got = _stage(xd, AHd, AWd, (b, C, T, H, W, (1, 1, 1), n, seed, p), 0, b * n, cpad)
    nb = L.lib().ivf_blob_count(T, T)
    frozen = torch.empty((b,) + tuple(got.shape[1:]), device='cuda')
    clip = torch.empty_like(frozen)
    zero = torch.zeros(b, T, device='cuda')
    for r in range(b):                                   # candidate nb - 1 of each clip: length T from frame 0
        L.check(L.lib().ivf_blob_stage(L.ptr(xd), b, C, T, H * W, T, 0, r * nb + nb - 1, 1, L.ptr(frozen[r]), cpad, L.stream()))
    L.check(L.lib().ivf_freeze_fwd(L.ptr(xd), L.ptr(zero), L.ptr(clip), b, C, T, H * W, 1, cpad, L.stream()))   # the clip in this layout
    torch.cuda.synchronize()
    bit = RR.bits(seed, p, n, 1)[:, 0]
    assert bit.any() and not bit.all()                   # both kinds occur
    for g in range(b * n):
        want = frozen[g // n] if bit[g % n] else clip[g // n]
        assert torch.equal(bits(got[g]), bits(want)), f"row {g} (bit {int(bit[g % n])})"
    assert not torch.equal(frozen, clip)


@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("T", [5, 16])
def test_a_rise_row_is_the_shapley_prefix_row_of_the_same_cells(T, cpad):
    """One scan for every grid-mask family: RISE mask k freezes f of the P cells; under the one-permutation rank table
    that ranks those cells 0 .. f-1 and the others f .. P-1, row f of ivf_shap_stage (n = 1) freezes the same cells and
    must be row k of ivf_rise_stage, bit for bit.  b = 1, C = 3, 12 x 20, grid (3, 3, 4), sigma 1.5, four masks."""
    import ivf_lib as L
    b, C, H, W, grid, n, seed, p = 1, 3, 12, 20, (3, 3, 4), 4, 1234, 0.5
    gt, gh, gw = grid
    P = gt * gh * gw
    xd = B.stage_inputs(b, C, T, H, W, key='rise').cuda()
    AHd, AWd = SR.axis_weights(H, gh, 1.5).cuda(), SR.axis_weights(W, gw, 1.5).cuda()
    rise = _stage(xd, AHd, AWd, (b, C, T, H, W, grid, n, seed, p), 0, n, cpad)
    compared = 0
    for k, frozen in enumerate(RR.bits(seed, p, n, P)):
        f = int(frozen.sum())
        if f == 0 or f == P:
            continue
        rank = np.empty(P, np.int64)
        rank[np.flatnonzero(frozen)] = np.arange(f)
        rank[np.flatnonzero(~frozen)] = np.arange(f, P)
        rkd = torch.from_numpy(rank.astype(np.uint16).view(np.int16)).cuda()
        buf, shap = guarded(tuple(rise.shape[1:]))
        bits(shap).fill_(NAN_BITS)
        L.check(L.lib().ivf_shap_stage(L.ptr(xd), b, C, T, H, W, L.ptr(AHd), L.ptr(AWd), gt, gh, gw, 1, L.ptr(rkd), f, 1,
                                       L.ptr(shap), cpad, L.stream()))
        torch.cuda.synchronize()
        assert untouched(buf)
        assert torch.equal(shap, rise[k]), f"mask {k} ({f} of {P} cells frozen): shap_stage row {f} is not rise_stage row {k}"
        compared += 1
    assert compared >= 3


# ---------------------------------------------------------------------------------------------------- plans
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


def _chain(eng, x, targets, grid, sigma, n, p, seed, math):
    """C.  rise_scores == st_perturbed_forward of the explicit expanded masks in the same chunk composition (equality);
    the rows of clip 1 of a two-clip call start at another place of their chunk: the other-composition gate"""
    b, T = x.shape[0], x.shape[2]
    Bp = eng.max_batch
    scores = eng.rise_scores(x, targets, n, p, grid, sigma, seed)
    assert tuple(scores.shape) == (b, n)
    S = torch.from_numpy(RR.frame_masks(RR.masks(seed, p, n, grid), T)).cuda()          # [n,T,gh,gw]
    assert torch.equal(eng.rise_masks(n, p, grid, seed), torch.from_numpy(RR.masks(seed, p, n, grid)).cuda())
    flat = scores.reshape(-1)
    tl = torch.as_tensor(targets, device='cuda').long()
    for first in range(0, b * n, Bp):
        rows = torch.arange(first, min(first + Bp, b * n), device='cuda')
        clip, k = rows // n, rows % n
        M = eng.st_expand(S[k].contiguous(), grid[1:], sigma)
        pr = eng.st_perturbed_forward(x[clip].contiguous(), M)[torch.arange(len(rows), device='cuda'), tl[clip]]
        assert torch.equal(pr, flat[first:first + len(rows)]), f"chunk at row {first}"
    assert len(torch.unique(flat)) > 1
    assert n % Bp != 0
    one = eng.rise_scores(x[1:].contiguous(), list(targets[1:]), n, p, grid, sigma, seed)
    e = rel_err_elem(scores[1:].cpu().numpy(), one.cpu().numpy(), FLOOR)
    assert e < _gate(math)
    return e


def test_i3d_rows_equal_st_perturbed_forward(s16):
    x = _s16_x((21, 7))
    targets = s16.argmax(s16.forward(x)).tolist()
    e = _chain(s16, x, targets, (2, 2, 2), 0.0, 40, 0.5, 1234, s16.math)
    note(f"rise chain I3D {s16.math}: 80 rows bit-equal to st_perturbed_forward; clip 1 at another chunk offset {e:.2e}")


def test_clstm_rows_equal_st_perturbed_forward(clstm):
    eng, c = clstm
    e = _chain(eng, c['x'].cuda(), _tg(c), (3,) + SR.CHAIN_GRID, SR.CHAIN_SIGMA, 13, 0.5, 1234, "fp32")
    note(f"rise chain ConvLSTM S2: rows bit-equal to st_perturbed_forward; clip 1 at another chunk offset {e:.2e}")


# ---------------------------------------------------------------------------------------------------- D. reduction
def _reduce(scores, orig, seed, p, grid):
    import ivf_lib as L
    s = torch.as_tensor(np.asarray(scores, np.float32)).cuda().contiguous()
    o = torch.as_tensor(np.asarray(orig, np.float32)).cuda().contiguous()
    b, n = s.shape
    bc, cells = guarded((b,) + grid)
    bn, cnt = guarded((b,) + grid, dtype=torch.int32, sent=-77)
    bm, md = guarded((b,))
    L.check(L.lib().ivf_rise_reduce(L.ptr(s), L.ptr(o), b, n, seed, RR.thresh(p), *grid, L.ptr(cells), L.ptr(cnt), L.ptr(md),
                                    L.stream()))
    torch.cuda.synchronize()
    assert untouched(bc) and untouched(bn, -77) and untouched(bm)
    return cells.cpu().numpy(), cnt.cpu().numpy(), md.cpu().numpy()


def _check_reduce(scores, orig, seed, p, grid, what):
    s32, o32 = np.asarray(scores, np.float32), np.asarray(orig, np.float32)
    got, cnt, md = _reduce(s32, o32, seed, p, grid)
    ref, rcnt, rmd, bound = RR.reduce_ref(s32, o32, seed, p, grid)
    assert np.array_equal(cnt, rcnt), f"{what}: counts differ"
    assert np.array_equal(np.isnan(got), rcnt == 0), f"{what}: NaN exactly where nothing is counted"
    ok = rcnt > 0
    err = np.abs(got.astype(np.float64) - ref)
    print(f"[rise reduce] {what}: worst err/bound {float((err[ok] / np.maximum(bound[ok], 1e-300)).max()) if ok.any() else 0.0:.3f}")
    assert bool((err[ok] <= bound[ok]).all()), f"{what}: cells off by {float((err[ok] - bound[ok]).max()):.3e} beyond the bound"
    # mean_drop: the same bound over all non-NaN masks of the clip
    d = o32.astype(np.float64)[:, None] - s32.astype(np.float64)
    nall = (~np.isnan(d)).sum(axis=1)
    mb = (nall + 2) * 2.0 ** -24 * np.nansum(np.abs(d), axis=1) / np.maximum(nall, 1)
    assert np.array_equal(np.isnan(md), nall == 0)
    assert bool((np.abs(md.astype(np.float64) - rmd)[nall > 0] <= mb[nall > 0]).all()), f"{what}: mean_drop"
    return got, cnt, ref


def test_reduction_against_fp64():
    g = np.random.default_rng(11)
    grid, n, b = (4, 3, 3), 64, 3
    s = g.random((b, n)).astype(np.float32)
    orig = np.array([0.9, 0.6, 0.3], np.float32)
    got, cnt, _ = _check_reduce(s, orig, 1234, 0.5, grid, "random scores")
    assert int(cnt.min()) == 22                                     # every clip sees the same masks
    # rows of a b-clip call == one-clip calls, bit for bit
    for r in range(b):
        one, c1, _ = _reduce(s[r:r + 1], orig[r:r + 1], 1234, 0.5, grid)
        assert np.array_equal(one.view(np.uint32), got[r:r + 1].view(np.uint32)) and np.array_equal(c1, cnt[r:r + 1])
    # NaN scores are neither summed nor counted: mask 5 leaves the cells it froze, and no other
    s2 = s.copy()
    s2[1, 5] = np.nan
    s2[2, :] = np.nan                                               # a clip with nothing left: NaN everywhere, count 0
    got2, cnt2, _ = _check_reduce(s2, orig, 1234, 0.5, grid, "NaN scores")
    froze = RR.bits(1234, 0.5, n, 36)[5].reshape(grid)
    assert froze.any() and not froze.all()
    assert np.array_equal(cnt[1] - cnt2[1], froze.astype(cnt.dtype))
    same = got2[1].view(np.uint32) == got[1].view(np.uint32)
    assert bool(same[~froze].all())
    assert np.array_equal(got2[0].view(np.uint32), got[0].view(np.uint32))
    assert np.isnan(got2[2]).all() and not cnt2[2].any()
    # the largest grid, p = 0.25, another seed
    _check_reduce(g.random((1, 9)).astype(np.float32), [0.7], 77, 0.25, (64, 32, 32), "64 x 32 x 32")


def test_reduction_uncounted_cells_are_nan():
    """n = 2 at p = 0.1 on 18 cells: the reference says which cells no mask froze"""
    g = np.random.default_rng(3)
    grid = (2, 3, 3)
    s = g.random((2, 2)).astype(np.float32)
    _, rcnt, _, _ = RR.reduce_ref(s, [0.5, 0.4], 1234, 0.1, grid)
    assert (rcnt == 0).any()
    got, cnt, _ = _check_reduce(s, [0.5, 0.4], 1234, 0.1, grid, "n = 2, p = 0.1")
    assert np.isnan(got).any()


@pytest.mark.parametrize("n,grid", [(16, (1, 3, 4)), (64, (4, 3, 3))])
def test_planted_cell_is_ranked_first_on_the_device(n, grid):
    cells = grid[0] * grid[1] * grid[2]
    planted = 7 % cells
    w = np.full(cells, 0.01)
    w[planted] = 0.5
    s = RR.planted_scores(1234, 0.5, n, grid, w).astype(np.float32)
    got, cnt, ref = _check_reduce(s, [0.9], 1234, 0.5, grid, f"planted cell, n = {n}")
    assert int(cnt.min()) >= 1
    assert int(np.argmax(ref.reshape(-1))) == planted               # the reference ranks it first ...
    assert int(np.argmax(got.reshape(-1))) == planted               # ... and so does the device


# ---------------------------------------------------------------------------------------------------- E. fixture
def test_s16_scores_vs_fixture(s16, golden):
    """the 16 masks of tests/golden/rise.npz within 1e-3 relative, each against its own magnitude; target bit-exact"""
    g = golden('rise')
    grid, n, p, seed = tuple(int(v) for v in g['grid']), int(g['n']), float(g['p']), int(g['seed'])
    assert (grid, n, p, seed, float(g['sigma']), int(g['clip'])) == ((2, 2, 2), 16, 0.5, 1234, 0.0, 21)
    x = _s16_x()
    t = int(torch.argmax(s16.forward(x)[0]))
    assert t == int(g['target'])                                    # integer output: bit-exact
    r = s16.rise(x, [t], n_masks=n, p=p, grid=grid, sigma=0.0, seed=seed)
    got = r["rise_scores"][0].cpu().numpy()
    e = rel_err_elem(got, g['scores'], FLOOR)
    eo = abs(float(r["score_x"][0]) - float(g['orig']))
    note(f"rise scores vs fixture {s16.math}: {n} masks, elementwise rel {e:.2e}, orig {eo:.2e} abs")
    assert e < 1e-3
    assert eo < 1e-3 * float(g['orig'])
    # the estimator on top: counts exact; a cell is a mean of orig - s_k, each term off by at most 1e-3 (orig + s_k)
    assert np.array_equal(r["rise_count"][0].cpu().numpy(), g['count'])
    Sb = RR.bits(seed, p, n, 8).reshape((n,) + grid)
    slack = 1e-3 * ((float(g['orig']) + g['scores'].astype(np.float64))[:, None, None, None] * Sb).sum(0) / g['count'] + 1e-6
    assert bool((np.abs(r["rise_cells"][0].cpu().numpy() - g['cells']) <= slack).all())
    assert tuple(r["rise_map"].shape) == (1, 16, 224, 224) and tuple(r["rise_frames"].shape) == (1, 16)


# ---------------------------------------------------------------------------------------------------- F. surfaces
def test_engine_rise_outputs(clstm):
    """rise() on the small ConvLSTM plan: the pieces agree with the entries they are made of"""
    import ivf_search
    eng, c = clstm
    x, tg = c['x'].cuda(), _tg(c)
    b, C, T, H, W = x.shape
    grid, sigma, n = (3,) + SR.CHAIN_GRID, SR.CHAIN_SIGMA, 13
    r = eng.rise(x, tg, n_masks=n, p=0.5, grid=grid, sigma=sigma, seed=9)
    assert set(r) == {"rise_scores", "rise_cells", "rise_count", "rise_mean_drop", "score_x", "rise_map", "rise_frames"}
    assert torch.equal(r["rise_scores"], eng.rise_scores(x, tg, n, 0.5, grid, sigma, 9))
    idx = torch.arange(b, device='cuda')
    assert torch.equal(r["score_x"], eng.forward(x)[idx, torch.as_tensor(tg, device='cuda')])
    cells, cnt, md = _reduce(r["rise_scores"].cpu().numpy(), r["score_x"].cpu().numpy(), 9, 0.5, grid)
    assert np.array_equal(cells.view(np.uint32), r["rise_cells"].cpu().numpy().view(np.uint32))
    assert np.array_equal(cnt, r["rise_count"].cpu().numpy()) and r["rise_count"].dtype == torch.int32
    assert np.array_equal(md.view(np.uint32), r["rise_mean_drop"].cpu().numpy().view(np.uint32))
    S = r["rise_cells"][:, torch.from_numpy(RR.frame_cell(T, grid[0])).cuda()].contiguous()
    assert torch.equal(r["rise_map"], eng.st_expand(S, grid[1:], sigma)) and tuple(r["rise_map"].shape) == (b, T, H, W)
    assert torch.equal(r["rise_frames"], ivf_search.frame_means(S))
    # b beyond max_batch: the same clips twice give the same rows twice
    x4 = torch.cat([x, x])
    r4 = eng.rise(x4, tg + tg, n_masks=n, p=0.5, grid=grid, sigma=sigma, seed=9)
    assert tuple(r4["rise_scores"].shape) == (2 * b, n) and tuple(r4["rise_cells"].shape) == (2 * b,) + grid
    for half in (r4["rise_scores"][:b], r4["rise_scores"][b:]):
        assert rel_err_elem(half.cpu().numpy(), r["rise_scores"].cpu().numpy(), FLOOR) < _gate("fp32")
    # the default grid: (min(T, 8),) + one cell per 32 input pixels
    assert tuple(eng.rise_masks(4).shape) == (4, min(T, 8), max(1, round(H / 32)), max(1, round(W / 32)))


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


def test_rise_video_i3d(smth_model):
    import ivf_recipe as RC
    from rise_videos import RiseVideo
    x = torch.from_numpy(RC.clip(21))[None]
    rv = RiseVideo(smth_model, n_masks=8, grid=(2, 2, 2), seed=3)
    m, out = rv(x)
    assert m.shape == (16, 224, 224) and m.dtype == np.float32 and tuple(out.shape) == (1, 174)
    assert np.isfinite(m).all() and m.any()
    eng = smth_model._engine_for(x.cuda(), min_batch=8)
    pred = int(torch.argmax(out[0]))
    want = eng.rise(x.cuda(), [pred], n_masks=8, grid=(2, 2, 2), seed=3)["rise_map"][0].cpu().numpy()
    assert np.array_equal(m.view(np.uint32), want.view(np.uint32))           # index None = the argmax
    m3, _ = RiseVideo(smth_model, n_masks=8, grid=(2, 2, 2), seed=3)(x, index=3)
    assert not np.array_equal(m3.view(np.uint32), m.view(np.uint32))
    assert set(rv.last) >= {"rise_scores", "rise_cells", "rise_count", "rise_mean_drop", "score_x", "rise_frames"}


def test_rise_video_clstm():
    import ivf_lib as L
    import ivf_recipe as RC
    from rise_videos import RiseVideo
    model = _kth_clstm()
    x = torch.from_numpy(RC.clip(7, 3, 32, 120, 160))[None]
    rv = RiseVideo(model, n_masks=12, p=0.5, grid=(4, 2, 3), seed=1, archType="CLSTM")
    m, out = rv(x, index=2)
    assert m.shape == (32, 120, 160) and m.dtype == np.float32 and tuple(out.shape) == (1, 6)
    assert tuple(rv.last["rise_cells"].shape) == (1, 4, 2, 3) and tuple(rv.last["rise_scores"].shape) == (1, 12)
    with pytest.raises(L.IvfError):
        RiseVideo(model, archType="VGG")(x)


RISE_KEYS = {'true_class', 'pred_class', 'video_id', 'RiseHeatMap', 'RiseCells', 'RiseCount', 'RiseFrames', 'rise_mean_drop',
             'n_masks', 'p', 'seed'}


def _check_rise_records(recs, tm, T, H, W, grid, n, nm, p, seed):
    assert len(recs) == len(tm) == n
    for rec, trec in zip(recs, tm):
        assert set(rec) == RISE_KEYS
        assert rec['RiseHeatMap'].shape == (T, H, W) and rec['RiseHeatMap'].dtype == np.float32
        assert rec['RiseCells'].shape == grid and rec['RiseCount'].shape == grid and rec['RiseFrames'].shape == (T,)
        assert rec['pred_class'] == trec['pred_class'] and rec['video_id'] is not None
        assert (rec['n_masks'], rec['p'], rec['seed']) == (nm, p, seed) and isinstance(rec['rise_mean_drop'], float)
        assert np.array_equal(rec['RiseCount'], RR.bits(seed, p, nm, grid[0] * grid[1] * grid[2]).sum(0).reshape(grid))


def test_smth_driver_with_rise(smth_model, tmp_path, monkeypatch):
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    loader = ivf_find_masks.SyntheticLoader(2, 2, (3, 16, 224, 224), 174, first_id=40)
    hp = {"batch_size": 2, "gradCamType": "guessed"}
    drv.find_masks(loader, smth_model, hp, 0.01, 0.02, 2, "central", "freeze", classOI=None, doGradCam=False,
                   runTempMask=True, verbose=False, doRise=True, riseMasks=8, riseProb=0.5, riseGrid=(2, 2, 2), riseSeed=5)
    tm = pickle.load(open(tmp_path / "results" / "allTimeMaskResults_run0_None_.p", "rb"))
    rs = pickle.load(open(tmp_path / "results" / "allRiseResults_run0_None_.p", "rb"))
    _check_rise_records(rs, tm, 16, 224, 224, (2, 2, 2), 2, 8, 0.5, 5)
    assert rs[0]['video_id'] == 40
    last = ivf_find_masks.find_masks_impl.last_rise_results
    assert len(last) == 2 and all(np.array_equal(a['RiseHeatMap'], q['RiseHeatMap']) for a, q in zip(last, rs))
    assert pickle.load(open(tmp_path / "results" / "allGradCamResults_run0_None_.p", "rb")) == []
    assert not (tmp_path / "results" / "allIntGradResults_run0_None_.p").exists()
    strips = [q for q in (tmp_path / "cam_saved_images").rglob("rise/*.png")]
    assert any(q.name == "casefreeze40_15.png" for q in strips) and any(q.name == "casereverse41_0.png" for q in strips)
    assert len(list((tmp_path / "cam_saved_images").rglob("rise/mygif.gif"))) == 2
    assert all(os.path.isdir(os.path.join(os.path.dirname(os.path.dirname(str(q))), "combined")) for q in strips)
    import ivf_lib as L
    with pytest.raises(L.IvfError):
        drv.find_masks(loader, smth_model, hp, 0.01, 0.02, 2, "central", "reverse", classOI=None, doGradCam=False,
                       runTempMask=True, verbose=False, doRise=True, riseMasks=8, riseGrid=(2, 2, 2))


def test_kth_driver_with_rise_on_the_convlstm(tmp_path, monkeypatch):
    import FindMasksComparison_I3D_KTH as drv
    import ivf_find_masks
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    loader = ivf_find_masks.SyntheticLoader(2, 2, (3, 32, 120, 160), 6, first_id=7)
    drv.find_masks(loader, _kth_clstm(), {"batch_size": 2, "gradCamType": "guessed"}, 0.02, 0.04, 2, 1, "central",
                   "freeze", classOI=None, doGradCam=False, runTempMask=True, verbose=False, doRise=True, riseMasks=12,
                   riseProb=0.5, riseGrid=(4, 2, 3), riseSeed=2)
    tm = pickle.load(open(tmp_path / "results" / "I3d_KTH_allTimeMaskResults_original_run0.p", "rb"))
    rs = pickle.load(open(tmp_path / "results" / "I3d_KTH_allRiseResults_original_run0.p", "rb"))
    _check_rise_records(rs, tm, 32, 120, 160, (4, 2, 3), 2, 12, 0.5, 2)
    assert all(np.isfinite(r_['RiseHeatMap']).all() for r_ in rs)          # every cell of this seed is counted
    assert rs[0]['video_id'] == "7"
    assert len(list((tmp_path / "cam_saved_images").rglob("rise/mygif.gif"))) == 2


def test_files_are_byte_identical_with_rise_off(smth_model, tmp_path, monkeypatch):
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    blobs = []
    for sub, extra in (("plain", {}), ("kwargs", dict(doRise=False, riseMasks=7, riseProb=0.3, riseGrid=(2, 2, 2), riseSigma=3.0,
                                                     riseSeed=9))):
        d = tmp_path / sub
        d.mkdir()
        monkeypatch.chdir(d)
        loader = ivf_find_masks.SyntheticLoader(1, 1, (3, 16, 224, 224), 174, first_id=40)
        drv.find_masks(loader, smth_model, {"batch_size": 1, "gradCamType": "guessed"}, 0.01, 0.02, 2, "central",
                       "freeze", classOI=None, doGradCam=True, runTempMask=True, verbose=False, **extra)
        files = sorted(q.relative_to(d) for q in d.rglob("*") if q.is_file())
        blobs.append({str(q): (d / q).read_bytes() for q in files})
        assert not any("Rise" in str(q) or "rise" in str(q) for q in files)
    assert blobs[0].keys() == blobs[1].keys()
    assert all(blobs[0][k] == blobs[1][k] for k in blobs[0]), [k for k in blobs[0] if blobs[0][k] != blobs[1][k]]


def test_refusals(clstm):
    import ivf_engine
    import ivf_lib as L
    import ivf_search
    eng, c = clstm
    x, tg = c['x'].cuda(), _tg(c)
    T = x.shape[2]
    for grid in ((T + 1, 3, 4), (0, 3, 4), (3, 33, 4), (3, 3, 0), (3, 4), "abc"):
        with pytest.raises(L.IvfError):
            eng.rise(x, tg, n_masks=4, grid=grid)
        with pytest.raises(L.IvfError):
            eng.rise_masks(4, grid=grid)
    for p in (0.0, 1.0, -0.5, 1.5, float('nan')):
        with pytest.raises(L.IvfError):
            eng.rise_scores(x, tg, 4, p, (3, 3, 4))
    with pytest.raises(L.IvfError):
        eng.rise(x, tg, n_masks=0, grid=(3, 3, 4))
    with pytest.raises(L.IvfError):
        eng.rise(x, tg, n_masks=4, grid=(3, 3, 4), seed=-1)
    with pytest.raises(L.IvfError):
        eng.rise(x, tg[:1], n_masks=4, grid=(3, 3, 4))                  # one target for two clips
    with pytest.raises(L.IvfError):
        ivf_search.MaskSearch(eng, mask_type="reverse", do_rise=True)
    ivf_search.MaskSearch(eng, mask_type="reverse")                     # off: 'reverse' stays what it was
    # the C entry: null pointers and a bad grid come back as error codes
    lib = L.lib()
    _, _, _, AH, AW = eng._st_axes((3, 4), 1.0)
    sc = torch.full((2, 4), -12345.0, device='cuda')
    tgt = torch.as_tensor(tg, dtype=torch.int32, device='cuda')
    fn = lib.ivf_clstm_rise_scores
    half = 1 << 31
    assert fn(eng._h, None, 2, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 3, 4, 4, 1, half, L.ptr(sc), L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 2, L.ptr(tgt), None, L.ptr(AW), 3, 3, 4, 4, 1, half, L.ptr(sc), L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 2, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 3, 4, 4, 1, half, None, L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 0, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 3, 4, 4, 1, half, L.ptr(sc), L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 2, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 3, 4, 4, 1, 0, L.ptr(sc), L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 2, L.ptr(tgt), L.ptr(AH), L.ptr(AW), T + 1, 3, 4, 4, 1, half, L.ptr(sc), L.stream()) == -1
    torch.cuda.synchronize()
    assert bool((sc == -12345.0).all())
    # the TF-style plan has no RISE entry and refuses
    tf = ivf_engine.TFCLSTMEngine(5, (1, 8, 30, 40), units=(4,), kernel=(3, 5), stride=2, padding="valid", max_batch=1)
    assert not hasattr(lib, "ivf_tfclstm_rise_scores")
    xt = torch.zeros(1, 1, 8, 30, 40, device='cuda')
    for call in (lambda: tf.rise(xt, [0], n_masks=4, grid=(2, 2, 2)), lambda: tf.rise_scores(xt, [0], 4, 0.5, (2, 2, 2)),
                 lambda: tf.rise_masks(4, grid=(2, 2, 2))):
        with pytest.raises(L.IvfError):
            call()
