"""Score-CAM (csrc/scorecam_ops.hip) on the GPU: the normalise kernel against the numpy float32
restatement (bits), the staging kernel against ivf_stmask_expand_fwd + ivf_stfreeze_fwd on the explicit per-frame S of
each row (equality) and 'blank' rows against torch's (1 - M) x, the score rows against st_perturbed_forward on both plans
and against tests/golden/scorecam.npz (make_golden_scorecam.py: the reference's I3D model under the torch restatement),
the reduction against the bounds of tests/scorecam_refs.py, and the public surfaces.  tests/test_scorecam_refs_host.py
proves the references on the CPU."""
import os
import pickle

import numpy as np
import pytest
import torch

import box_refs as B
import scorecam_refs as SC
import stmask_refs as SR
from conftest import note, rel_err_elem
from test_gpu_box import FLOOR, _gate
from test_gpu_leaf_kernels import bits, guarded, untouched

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00ABC

# Gate (b) of the fixture test: 4x the worst relative error of scorecam_cam against the fixture's cam measured in the
# first GPU run of this test (profiles/scorecam_bench.txt), and never more than 1e-2.
CAM_VS_FIXTURE_MEASURED = 1.80e-6
CAM_VS_FIXTURE_GATE = min(4 * CAM_VS_FIXTURE_MEASURED, 1e-2)


# ---------------------------------------------------------------------------------------------------- A. normalise
def _planes(b, nc, cells, seed):
    g = np.random.default_rng(seed)
    A = g.standard_normal((b, nc, cells)).astype(np.float32)
    if nc >= 5:
        A[0, 1] = 0.25                                   # constant
        A[0, 2, cells // 2] = np.nan
        A[1, 0, 0] = np.inf
        A[1, 3, cells - 1] = -np.inf
        A[1, 4] = np.maximum(A[1, 4], 0)                 # a ReLU plane
    return A


@pytest.mark.parametrize("cells", [1, 98, 6272])
@pytest.mark.parametrize("nc", [1, 5, 130])
def test_normalise_is_the_float32_restatement(nc, cells):
    import ivf_lib as L
    b = 2
    A = _planes(b, nc, cells, 100 * nc + cells)
    Ad = torch.from_numpy(A).cuda()
    bl, lo = guarded((b, nc))
    bh, hi = guarded((b, nc))
    bv, valid = guarded((b, nc), dtype=torch.int32, sent=-77)
    bf, F = guarded((b, nc, cells))
    bits(F).fill_(NAN_BITS)
    L.check(L.lib().ivf_scorecam_normalise(L.ptr(Ad), b, nc, cells, L.ptr(lo), L.ptr(hi), L.ptr(valid), L.ptr(F), L.stream()))
    torch.cuda.synchronize()
    assert untouched(bl) and untouched(bh) and untouched(bv, -77) and untouched(bf)
    rlo, rhi, rvalid, rF = SC.normalise(A)
    assert np.array_equal(lo.cpu().numpy().view(np.uint32), rlo.view(np.uint32))
    assert np.array_equal(hi.cpu().numpy().view(np.uint32), rhi.view(np.uint32))
    assert np.array_equal(valid.cpu().numpy(), rvalid.astype(np.int32))
    assert np.array_equal(F.cpu().numpy().view(np.uint32), rF.view(np.uint32))
    if cells == 1:
        assert not rvalid.any() and bool((F == 1).all())            # a one-cell plane is constant
    elif nc >= 5:
        want = np.ones((b, nc), bool)
        want[0, 1] = want[0, 2] = want[1, 0] = want[1, 3] = False
        assert np.array_equal(rvalid, want) and bool((F.cpu()[torch.from_numpy(~want)] == 1).all())
    else:
        assert rvalid.all()


# ---------------------------------------------------------------------------------------------------- B. staging
def _layout(t, cpad):
    """[n,C,T,H,W] -> the staged layout"""
    n, C, T, H, W = t.shape
    if cpad == 0:
        return t.reshape(n, C, T, H * W).contiguous()
    out = torch.zeros(n, T, H * W, 4, device=t.device)
    out[..., :C] = t.permute(0, 2, 3, 4, 1).reshape(n, T, H * W, C)
    return out


def _stage(xd, AHd, AWd, Fd, perturb, first, count, cpad):
    import ivf_lib as L
    b, C, T, H, W = xd.shape
    nc, gt, gh, gw = Fd.shape[1:]
    buf, out = guarded((count, C, T, H * W) if cpad == 0 else (count, T, H * W, 4))
    bits(out).fill_(NAN_BITS)
    L.check(L.lib().ivf_scorecam_stage(L.ptr(xd), b, C, T, H, W, L.ptr(AHd), L.ptr(AWd), gt, gh, gw, L.ptr(Fd), nc, perturb,
                                       first, count, L.ptr(out), cpad, L.stream()))
    torch.cuda.synchronize()
    assert untouched(buf), f"scorecam_stage out_cpad={cpad}: a sentinel row was written"
    assert not bool(torch.isnan(out).any()), f"scorecam_stage out_cpad={cpad}: an element was never written"
    return out


def _want(xd, AHd, AWd, Fd, S_all, perturb, first, count, cpad):
    """the same rows: channel rows by ivf_stmask_expand_fwd (+ ivf_stfreeze_fwd, or torch's (1 - M) x under 'blank') on
    the explicit per-frame S, baseline rows the clip with every frame = frame 0 (or +0.0 under 'blank')"""
    import ivf_lib as L
    b, C, T, H, W = xd.shape
    nc, gt, gh, gw = Fd.shape[1:]
    rows = np.arange(first, first + count)
    clip, k = rows // (nc + 1), rows % (nc + 1)
    base = torch.from_numpy(k == nc).cuda()
    xr = xd[torch.from_numpy(clip).cuda()].contiguous()
    S = S_all[torch.from_numpy(clip).cuda(), torch.from_numpy(np.minimum(k, nc - 1)).cuda()].contiguous()    # [count,T,gh,gw]
    M = torch.empty(count, T, H, W, device='cuda')
    L.check(L.lib().ivf_stmask_expand_fwd(L.ptr(S), L.ptr(AHd), L.ptr(AWd), L.ptr(M), count, T, gh, gw, H, W, L.stream()))
    if perturb == 0:
        out = torch.empty((count, C, T, H * W) if cpad == 0 else (count, T, H * W, 4), device='cuda')
        L.check(L.lib().ivf_stfreeze_fwd(L.ptr(xr), L.ptr(M), L.ptr(out), count, C, T, H * W, cpad, L.stream()))
        frozen = _layout(xr[:, :, :1].expand(-1, -1, T, -1, -1).contiguous(), cpad)
    else:
        out = _layout((1.0 - M)[:, None] * xr, cpad)
        frozen = torch.zeros_like(out)
    torch.cuda.synchronize()
    out[base] = frozen[base]
    return out, xr


def _check_windows(C, T, sigma, grid, cpad, perturb, windows, H=9, W=21, b=2, nc=5):
    gt, gh, gw = grid
    xd = B.stage_inputs(b, C, T, H, W, key='scorecam').cuda()
    AHd, AWd = SR.axis_weights(H, gh, sigma).cuda(), SR.axis_weights(W, gw, sigma).cuda()
    g = np.random.default_rng(gt * 1000 + gh * 37 + gw)
    F = g.random((b, nc, gt, gh, gw)).astype(np.float32)
    F.reshape(b, nc, -1)[:, :, 0] = 0.0                              # the cells lo and hi map to
    F.reshape(b, nc, -1)[:, 1:, -1] = 1.0
    Fd = torch.from_numpy(F).cuda()
    S_all = torch.from_numpy(SC.frame_planes(F, T)).cuda()           # [b,nc,T,gh,gw]
    per, moved, got_all = nc + 1, 0, {}
    for first, count in windows:
        assert 0 <= first and first + count <= b * per
        got = _stage(xd, AHd, AWd, Fd, perturb, first, count, cpad)
        want, xr = _want(xd, AHd, AWd, Fd, S_all, perturb, first, count, cpad)
        assert torch.equal(bits(got), bits(want)), \
            f"rows [{first}, {first + count}) of {b * per}, perturb {perturb}: not the bits of the explicit pair"
        if cpad == 4:
            assert torch.equal(bits(got[..., C:]), torch.zeros_like(bits(got[..., C:]))), "pad lane not +0.0"
        moved += int((got != _layout(xr, cpad)).flatten(1).any(dim=1).sum())
        got_all[(first, count)] = got
    assert moved > 0, "no staged row differs from its clip: the comparison is vacuous"
    return xd, AHd, AWd, Fd, got_all


# windows of the 12 rows of two clips (nc = 5): mid-clip, across the clip boundary with the baseline row 5, ending on
# the last baseline row, the whole list
WINDOWS = [(2, 3), (4, 4), (9, 3), (0, 12)]
GRIDS = [(1, 1, 1), (2, 3, 4), (None, 1, 1), (3, 32, 32)]


@pytest.mark.parametrize("perturb", [0, 1])
@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("sigma", [0.0, 12.0])
@pytest.mark.parametrize("C", [1, 3])
def test_staging_is_expand_plus_freeze_on_the_explicit_planes(C, sigma, cpad, perturb):
    """B.  b = 2, T = 5, 9 x 21 (one workgroup with 67 idle threads), the four grids, nc = 5; a row of the two-clip call
    is the one-clip call's row"""
    T = 5
    for grid in GRIDS:
        grid = (T if grid[0] is None else grid[0],) + grid[1:]
        xd, AHd, AWd, Fd, got = _check_windows(C, T, sigma, grid, cpad, perturb, WINDOWS)
        one = _stage(xd[1:].contiguous(), AHd, AWd, Fd[1:].contiguous(), perturb, 0, 6, cpad)
        assert torch.equal(bits(one), bits(got[(0, 12)][6:])), f"grid {grid}: clip 1 alone differs from clip 1 of two"


@pytest.mark.parametrize("perturb", [0, 1])
@pytest.mark.parametrize("cpad", [0, 4])
def test_staging_over_several_workgroups(cpad, perturb):
    """19 x 37 = 703 pixels: three workgroups per row, the last ragged, rows of pixels that straddle workgroups"""
    _check_windows(3, 6, 1.0, (2, 3, 4), cpad, perturb, [(3, 5), (0, 8)], H=19, W=37, nc=3)
    _check_windows(2, 3, 0.0, (3, 2, 32), cpad, perturb, [(1, 5)], H=19, W=37, nc=2)


@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("T", [5, 16, 17, 32])
def test_staging_on_every_frame_count_path(T, cpad):
    """B at T = 5 and 17 (the frame loop) and T = 16 and 32 (pieces of 16 preloaded frames), with two temporal cells and
    one per frame, both perturbations"""
    for gt in (2, T):
        for perturb in (0, 1):
            _check_windows(3, T, 1.5, (gt, 3, 4), cpad, perturb, [(4, 4), (9, 3)])


@pytest.mark.parametrize("cpad", [0, 4])
def test_staging_with_the_largest_plane(cpad):
    """8 x 32 x 32 = 8192 cells: the whole 32 KiB of the plane beside the 32 KiB of A_W columns"""
    _check_windows(3, 16, 0.0, (8, 32, 32), cpad, 0, [(1, 3)], nc=2)


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


def _chain(eng, x, targets, layer, channels, sigma):
    """C.  every score == st_perturbed_forward of the row's explicit expanded mask (the baseline row: M == 1) in the
    same chunk composition, by bits"""
    b, T = x.shape[0], x.shape[2]
    Bp = eng.max_batch
    planes = eng.scorecam_planes(x, layer, channels)
    F = planes["F"]
    nc, gt, gh, gw = F.shape[1:]
    per = nc + 1
    scores = eng.scorecam_scores(x, targets, F, sigma, "freeze")
    assert tuple(scores.shape) == (b, per)
    kt = torch.from_numpy(SC.frame_cell(T, gt)).cuda()
    S = torch.cat([F[:, :, kt], torch.ones(b, 1, T, gh, gw, device='cuda')], dim=1).reshape(b * per, T, gh, gw)
    flat = scores.reshape(-1)
    tl = torch.as_tensor(targets, device='cuda').long()
    for first in range(0, b * per, Bp):
        rows = torch.arange(first, min(first + Bp, b * per), device='cuda')
        clip = rows // per
        M = eng.st_expand(S[rows].contiguous(), (gh, gw), sigma)
        M[rows % per == nc] = 1.0                                    # the baseline row's M is 1 exactly, not the expanded ones
        pr = eng.st_perturbed_forward(x[clip].contiguous(), M)[torch.arange(len(rows), device='cuda'), tl[clip]]
        assert torch.equal(bits(pr), bits(flat[first:first + len(rows)])), f"chunk at row {first}"
    assert len(torch.unique(flat)) > 1
    return planes, scores


def test_i3d_rows_equal_st_perturbed_forward(s16):
    x = _s16_x((21, 7))
    targets = s16.argmax(s16.forward(x)).tolist()
    planes, scores = _chain(s16, x, targets, "Mixed_5c", (100, 11), 0.0)
    assert (2 * 12) % s16.max_batch != 0 and tuple(planes["A"].shape) == (2, 11, 2, 7, 7)
    note(f"scorecam chain I3D {s16.math}: 24 rows bit-equal to st_perturbed_forward, "
         f"{int(planes['valid'].sum())} of 22 channels valid")


def test_clstm_rows_equal_st_perturbed_forward(clstm):
    eng, c = clstm
    x = c['x'].cuda()
    planes, scores = _chain(eng, x, _tg(c), 0, None, SR.CHAIN_SIGMA)
    assert planes["A"].shape[2] == x.shape[2]                       # 'cell0': one map per frame
    x3 = torch.cat([x, x[:1]])                                       # b beyond max_batch: the same clip gives the same row
    s3 = eng.scorecam_scores(x3, _tg(c) + _tg(c)[:1], torch.cat([planes["F"], planes["F"][:1]]), SR.CHAIN_SIGMA)
    assert tuple(s3.shape) == (x.shape[0] + 1, scores.shape[1])
    assert rel_err_elem(s3[-1].cpu().numpy(), scores[0].cpu().numpy(), FLOOR) < _gate("fp32")   # another chunk offset
    note(f"scorecam chain ConvLSTM S2 cell0: {scores.numel()} rows bit-equal to st_perturbed_forward")


# ---------------------------------------------------------------------------------------------------- D. reduction
def _reduce(scores, A, valid, kind):
    import ivf_lib as L
    s = torch.as_tensor(np.asarray(scores, np.float32)).cuda().contiguous()
    Ad = torch.as_tensor(np.asarray(A, np.float32)).cuda().contiguous()
    v = torch.as_tensor(np.asarray(valid).astype(np.int32)).cuda().contiguous()
    b, nc, cells = Ad.shape
    bw, w = guarded((b, nc))
    bc, cam = guarded((b, cells))
    bits(w).fill_(NAN_BITS)
    bits(cam).fill_(NAN_BITS)
    L.check(L.lib().ivf_scorecam_reduce(L.ptr(s), L.ptr(Ad), L.ptr(v), b, nc, cells, kind, L.ptr(w), L.ptr(cam), L.stream()))
    torch.cuda.synchronize()
    assert untouched(bw) and untouched(bc)
    return w.cpu().numpy(), cam.cpu().numpy()


def _check_reduce(scores, A, valid, what):
    out = {}
    for kind, name in ((0, "increase"), (1, "softmax")):
        w, cam = _reduce(scores, A, valid, kind)
        d, ok = SC.counting(scores, valid)
        assert np.array_equal(w[~ok].view(np.uint32), np.zeros(int((~ok).sum()), np.uint32)), f"{what} {name}: weight not +0.0"
        if kind == 0:
            assert np.array_equal(w.view(np.uint32), SC.weights_increase(scores, valid).view(np.uint32)), f"{what}: increase"
        else:
            ref, rel = SC.weights_softmax(scores, valid)
            err = np.abs(w.astype(np.float64) - ref)
            print(f"[scorecam reduce] {what} softmax: worst err/bound "
                  f"{float((err / np.maximum(rel[:, None] * ref, 1e-300))[ok].max()) if ok.any() else 0.0:.3f}")
            assert bool((err <= rel[:, None] * ref).all()), f"{what}: softmax weights beyond the bound"
        ref, bound = SC.cam_ref(w, A)
        err = np.abs(cam.astype(np.float64) - ref)
        print(f"[scorecam reduce] {what} {name}: cam worst err/bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), f"{what} {name}: cam off by {float((err - bound).max()):.3e} beyond the bound"
        assert bool((cam >= 0).all())
        out[name] = (w, cam, ref)
    return out


@pytest.mark.parametrize("cells", [1, 98])
@pytest.mark.parametrize("nc", [1, 7, 1024])
def test_reduction_against_the_bounds(nc, cells):
    g = np.random.default_rng(nc + cells)
    b = 3
    s = g.random((b, nc + 1)).astype(np.float32)
    A = g.standard_normal((b, nc, cells)).astype(np.float32)
    valid = np.ones((b, nc), bool)
    full = _check_reduce(s, A, valid, f"nc {nc} cells {cells}")
    for r in range(b):                                               # rows of a b-clip call == one-clip calls, bit for bit
        w1, c1 = _reduce(s[r:r + 1], A[r:r + 1], valid[r:r + 1], 1)
        assert np.array_equal(w1.view(np.uint32), full["softmax"][0][r:r + 1].view(np.uint32))
        assert np.array_equal(c1.view(np.uint32), full["softmax"][1][r:r + 1].view(np.uint32))
    if nc >= 7:
        s2, A2, v2 = s.copy(), A.copy(), valid.copy()
        s2[0, 3] = np.nan                                            # a NaN score: weight 0
        v2[1, 2] = False                                             # a channel that is not valid: weight 0, and its
        A2[1, 2] = np.nan                                            # plane never reaches the map
        s2[2, nc] = np.nan                                           # a NaN baseline: nothing counts, the map is 0
        out = _check_reduce(s2, A2, v2, f"nc {nc} cells {cells}, NaN and invalid")
        for name in ("increase", "softmax"):
            w, cam, _ = out[name]
            assert w[0, 3] == 0 and w[1, 2] == 0 and not w[2].any() and not cam[2].any() and np.isfinite(cam).all()


def test_planted_channel_is_the_argmax_on_the_device():
    g = np.random.default_rng(8)
    nc, shape = 7, (2, 7, 7)
    A = (0.1 * g.random((1, nc) + shape)).astype(np.float32)
    A[0, 3] = 0
    A[0, 3, 1, 4, 2] = 5.0
    s = np.full((1, nc + 1), 0.2, np.float32)
    s[0, 3] = 0.9
    hot = (1 * 7 + 4) * 7 + 2
    out = _check_reduce(s, A.reshape(1, nc, -1), np.ones((1, nc), bool), "planted channel")
    for name in ("increase", "softmax"):
        w, cam, ref = out[name]
        assert int(np.argmax(ref.reshape(-1))) == hot               # the reference ranks it first ...
        assert int(np.argmax(cam.reshape(-1))) == hot               # ... and so does the device


# ---------------------------------------------------------------------------------------------------- E. fixture
def test_s16_vs_fixture(s16, golden):
    """(a) the fixture's own F through ivf_i3d_scorecam_scores: the 25 scores of tests/golden/scorecam.npz within 1e-3
    relative, each against its own magnitude, the target bit-exact.  (b) end to end from the device's own activations:
    the worst error of scorecam_cam against the fixture's fp64 cam, relative to the cam's maximum (the min/max
    normalisation divides by a range, which amplifies the activations' own error; the gate is 4x the figure of the first
    GPU run and at most 1e-2)."""
    g = golden('scorecam')
    first, count = int(g['first']), int(g['count'])
    assert (int(g['clip']), first, count, float(g['sigma'])) == (21, 100, 24, 0.0) and int(g['valid'].sum()) >= 16
    x = _s16_x()
    t = int(torch.argmax(s16.forward(x)[0]))
    assert t == int(g['target'])                                    # integer output: bit-exact
    F = torch.from_numpy(g['F'])[None].cuda()
    got = s16.scorecam_scores(x, [t], F, 0.0, "freeze")[0].cpu().numpy()
    e = rel_err_elem(got, g['scores'], FLOOR)
    note(f"scorecam scores vs fixture {s16.math}: {count + 1} rows from the fixture's F, elementwise rel {e:.2e}")
    assert e < 1e-3
    # the 'softmax' map: the 'increase' weights are signed and their map on this clip is 0 everywhere after the relu
    r = s16.scorecam(x, [t], layer="Mixed_5c", weights="softmax", perturb="freeze", sigma=0.0, channels=(first, count))
    assert np.array_equal(r["scorecam_valid"][0].cpu().numpy().astype(bool), g['valid'])
    cam = r["scorecam_cam"][0].cpu().numpy().astype(np.float64)
    ec = float(np.abs(cam - g['cam_softmax']).max() / g['cam_softmax'].max())
    ew = rel_err_elem(r["scorecam_weights"][0].cpu().numpy(), g['w_softmax'], 1e-3)
    note(f"scorecam softmax weights vs fixture {s16.math}: elementwise rel {ew:.2e}")
    ea = rel_err_elem(s16.scorecam_planes(x, "Mixed_5c", (first, count))["A"][0].cpu().numpy(), g['A'], float(np.abs(g['A']).max()))
    note(f"scorecam end to end vs fixture {s16.math}: cam worst rel {ec:.2e} (gate {CAM_VS_FIXTURE_GATE:.1e}), "
         f"activations {ea:.2e}")
    assert ec < CAM_VS_FIXTURE_GATE
    assert tuple(r["scorecam_map"].shape) == (1, 16, 224, 224) and tuple(r["scorecam_scores"].shape) == (1, count + 1)


# ---------------------------------------------------------------------------------------------------- F. surfaces
def test_engine_scorecam_outputs(clstm):
    """scorecam() on the small ConvLSTM plan: the pieces agree with the entries they are made of"""
    import ivf_lib as L
    eng, c = clstm
    x, tg = c['x'].cuda(), _tg(c)
    b, C, T, H, W = x.shape
    for layer, weights, perturb in ((0, "increase", "freeze"), (None, "softmax", "blank")):
        r = eng.scorecam(x, tg, layer=layer, weights=weights, perturb=perturb, sigma=SR.CHAIN_SIGMA)
        assert set(r) == {"scorecam_map", "scorecam_cam", "scorecam_weights", "scorecam_scores", "scorecam_valid", "score_x",
                          "score_base"}
        planes = eng.scorecam_planes(x, layer)
        nc, gt, gh, gw = planes["A"].shape[1:]
        assert torch.equal(r["scorecam_valid"], planes["valid"]) and r["scorecam_valid"].dtype == torch.int32
        scores = eng.scorecam_scores(x, tg, planes["F"], SR.CHAIN_SIGMA, perturb)
        assert torch.equal(bits(r["scorecam_scores"]), bits(scores)) and torch.equal(r["score_base"], scores[:, -1])
        w, cam = eng.scorecam_reduce(scores, planes["A"], planes["valid"], weights)
        assert torch.equal(bits(r["scorecam_weights"]), bits(w)) and torch.equal(bits(r["scorecam_cam"]), bits(cam))
        idx = torch.arange(b, device='cuda')
        assert torch.equal(r["score_x"], eng.forward(x)[idx, torch.as_tensor(tg, device='cuda')])
        step = T // gt
        out = torch.empty(b, gt * step, H, W, device='cuda')
        mm = torch.empty(b, gt, 2, device='cuda')
        L.check(L.lib().ivf_cam_resize_normalise(L.ptr(cam), L.ptr(out), L.ptr(mm), b, gt, gh, gw, H, W, step, 1, L.stream()))
        torch.cuda.synchronize()
        assert torch.equal(bits(r["scorecam_map"]), bits(out))
        gc, _ = eng.gradcam(x, tg, layer=layer)
        assert r["scorecam_map"].shape == gc.shape                  # Grad-CAM's shape for the same target
    # a window of channels is that window of the whole layer's planes
    whole = eng.scorecam_planes(x, 0)
    part = eng.scorecam_planes(x, 0, (1, 2))
    assert torch.equal(bits(part["F"]), bits(whole["F"][:, 1:3].contiguous())) and tuple(part["A"].shape[:2]) == (b, 2)


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


def test_scorecam_video_i3d(smth_model):
    import ivf_lib as L
    import ivf_recipe as RC
    from scorecam_videos import ScoreCamVideo
    x = torch.from_numpy(RC.clip(21))[None]
    sv = ScoreCamVideo(smth_model, ["Mixed_5c"], None, True, 224, True, channels=(100, 8), sigma=0.0)
    m, out = sv(x)
    assert m.shape == (16, 224, 224) and m.dtype == np.float32 and tuple(out.shape) == (1, 174)
    eng = smth_model._engine_for(x.cuda(), min_batch=9)
    pred = int(torch.argmax(out[0]))
    want = eng.scorecam(x.cuda(), [pred], layer="Mixed_5c", channels=(100, 8), sigma=0.0)["scorecam_map"][0].cpu().numpy()
    assert np.array_equal(m.view(np.uint32), want.view(np.uint32))           # index None = the argmax
    assert set(sv.last) >= {"scorecam_cam", "scorecam_weights", "scorecam_scores", "scorecam_valid", "score_x", "score_base"}
    assert tuple(sv.last["scorecam_scores"].shape) == (1, 9)
    # refusals: a layer whose map is too large, a bad weights / perturb name, channels outside the layer, two clips
    with pytest.raises(L.IvfError, match="exceeds the limits"):
        ScoreCamVideo(smth_model, ["Conv3d_2c_3x3"], None, True, channels=(0, 8))(x)
    for name in ("Conv3d_1a_7x7", "MaxPool3d_2a_3x3", "Conv3d_2b_1x1"):
        with pytest.raises(L.IvfError, match="exceeds the limits"):
            eng.scorecam_planes(x.cuda(), name, (0, 2))
    assert eng._scorecam_layer("MaxPool3d_3a_3x3", None)[3:6] == (8, 28, 28)
    with pytest.raises(L.IvfError, match="weights"):
        ScoreCamVideo(smth_model, ["Mixed_5c"], None, True, weights="mean", channels=(0, 8))(x)
    with pytest.raises(L.IvfError, match="perturb"):
        ScoreCamVideo(smth_model, ["Mixed_5c"], None, True, perturb="reverse", channels=(0, 8))(x)
    for ch in ((1020, 8), (-1, 4), (0, 0), "ab"):
        with pytest.raises(L.IvfError):
            ScoreCamVideo(smth_model, ["Mixed_5c"], None, True, channels=ch)(x)
    with pytest.raises(L.IvfError, match="one clip"):
        ScoreCamVideo(smth_model, ["Mixed_5c"], None, True, channels=(0, 8))(torch.cat([x, x]))
    with pytest.raises(L.IvfError):
        L.cam_kind_ids(["scorecam"])                                 # still not a kind of GradCamVideo


def test_scorecam_video_clstm():
    import ivf_lib as L
    import ivf_recipe as RC
    from scorecam_videos import ScoreCamVideo
    model = _kth_clstm()
    x = torch.from_numpy(RC.clip(7, 3, 32, 120, 160))[None]
    sv = ScoreCamVideo(model, ["cell1"], None, True, (160, 120), True, weights="softmax", archType="CLSTM")
    m, out = sv(x, index=2)
    assert m.shape == (32, 120, 160) and m.dtype == np.float32 and tuple(out.shape) == (1, 6)
    eng = model._engine_for(x.cuda())
    want = eng.scorecam(x.cuda(), [2], layer=1, weights="softmax")["scorecam_map"][0].cpu().numpy()
    assert np.array_equal(m.view(np.uint32), want.view(np.uint32))
    assert tuple(sv.last["scorecam_scores"].shape) == (1, 5) and tuple(sv.last["scorecam_cam"].shape[:2]) == (1, 32)
    m2, _ = ScoreCamVideo(model, ["clstm"], None, True, (160, 120), True, archType="CLSTM")(x, index=2)
    assert m2.shape == (32, 120, 160)                                # 4 effective steps, each repeated 8 times
    with pytest.raises(L.IvfError, match="exceeds the limits"):
        ScoreCamVideo(model, ["cell0"], archType="CLSTM")(x)         # a 30 x 40 map: wider than 32 cells
    with pytest.raises(L.IvfError):
        ScoreCamVideo(model, ["cell1"], archType="VGG")(x)
    with pytest.raises(L.IvfError):
        ScoreCamVideo(model, ["cell7"], archType="CLSTM")(x)


SC_KEYS = {'true_class', 'pred_class', 'video_id', 'ScoreCamHeatMap', 'ScoreCamWeights', 'ScoreCamValid', 'score_base',
           'layer', 'weights', 'perturb'}


def _check_records(recs, tm, shape, nc):
    assert len(recs) == len(tm) == 2
    for rec, trec in zip(recs, tm):
        assert set(rec) == SC_KEYS
        assert rec['ScoreCamHeatMap'].shape == shape and rec['ScoreCamHeatMap'].dtype == np.float32
        assert rec['ScoreCamWeights'].shape == (nc,) and rec['ScoreCamValid'].shape == (nc,)
        assert rec['pred_class'] == trec['pred_class'] and isinstance(rec['score_base'], float)
        assert (rec['weights'], rec['perturb']) == ("increase", "freeze")


def test_smth_driver_with_scorecam(smth_model, tmp_path, monkeypatch):
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    loader = ivf_find_masks.SyntheticLoader(2, 2, (3, 16, 224, 224), 174, first_id=40)
    hp = {"batch_size": 2, "gradCamType": "guessed"}
    drv.find_masks(loader, smth_model, hp, 0.01, 0.02, 2, "central", "freeze", classOI=None, doGradCam=False,
                   runTempMask=True, verbose=False, doScoreCam=True, scoreCamChannels=(0, 8), doCurves=True)
    tm = pickle.load(open(tmp_path / "results" / "allTimeMaskResults_run0_None_.p", "rb"))
    rs = pickle.load(open(tmp_path / "results" / "allScoreCamResults_run0_None_.p", "rb"))
    _check_records(rs, tm, (16, 224, 224), 8)
    assert rs[0]['video_id'] == 40 and rs[0]['layer'] is None
    last = ivf_find_masks.find_masks_impl.last_scorecam_results
    assert len(last) == 2 and all(np.array_equal(a['ScoreCamHeatMap'], q['ScoreCamHeatMap'], equal_nan=True)
                                  for a, q in zip(last, rs))
    cv = pickle.load(open(tmp_path / "results" / "allCurvesResults_run0_None_.p", "rb"))
    assert all('scorecam' in rec and rec['scorecam']['deletion'].shape == (17,) for rec in cv)
    assert pickle.load(open(tmp_path / "results" / "allGradCamResults_run0_None_.p", "rb")) == []
    strips = [q for q in (tmp_path / "cam_saved_images").rglob("scorecam/*.png")]
    assert any(q.name == "casefreeze40_15.png" for q in strips) and any(q.name == "casereverse41_0.png" for q in strips)
    assert all(os.path.isdir(os.path.join(os.path.dirname(os.path.dirname(str(q))), "combined")) for q in strips)


def test_kth_driver_with_scorecam_on_the_convlstm(tmp_path, monkeypatch):
    import FindMasksComparison_I3D_KTH as drv
    import ivf_find_masks
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    loader = ivf_find_masks.SyntheticLoader(2, 2, (3, 32, 120, 160), 6, first_id=7)
    drv.find_masks(loader, _kth_clstm(), {"batch_size": 2, "gradCamType": "guessed"}, 0.02, 0.04, 2, 1, "central",
                   "freeze", classOI=None, doGradCam=False, runTempMask=True, verbose=False, doScoreCam=True,
                   scoreCamTarget=1, scoreCamChannels=(0, 4), doCurves=True)
    tm = pickle.load(open(tmp_path / "results" / "I3d_KTH_allTimeMaskResults_original_run0.p", "rb"))
    rs = pickle.load(open(tmp_path / "results" / "I3d_KTH_allScoreCamResults_original_run0.p", "rb"))
    _check_records(rs, tm, (32, 120, 160), 4)
    assert rs[0]['video_id'] == "7" and rs[0]['layer'] == 1
    cv = pickle.load(open(tmp_path / "results" / "I3d_KTH_allCurvesResults_original_run0.p", "rb"))
    assert all('scorecam' in rec for rec in cv)


def test_files_are_byte_identical_with_scorecam_off(smth_model, tmp_path, monkeypatch):
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    blobs = []
    for sub, extra in (("plain", {}), ("kwargs", dict(doScoreCam=False, scoreCamTarget="Mixed_4f", scoreCamWeights="softmax",
                                                     scoreCamPerturb="blank", scoreCamSigma=3.0, scoreCamChannels=(0, 8)))):
        d = tmp_path / sub
        d.mkdir()
        monkeypatch.chdir(d)
        loader = ivf_find_masks.SyntheticLoader(1, 1, (3, 16, 224, 224), 174, first_id=40)
        drv.find_masks(loader, smth_model, {"batch_size": 1, "gradCamType": "guessed"}, 0.01, 0.02, 2, "central",
                       "freeze", classOI=None, doGradCam=True, runTempMask=True, verbose=False, **extra)
        files = sorted(q.relative_to(d) for q in d.rglob("*") if q.is_file())
        blobs.append({str(q): (d / q).read_bytes() for q in files})
        assert not any("ScoreCam" in str(q) or "scorecam" in str(q) for q in files)
    assert blobs[0].keys() == blobs[1].keys()
    assert all(blobs[0][k] == blobs[1][k] for k in blobs[0]), [k for k in blobs[0] if blobs[0][k] != blobs[1][k]]


def test_refusals(clstm):
    import ivf_engine
    import ivf_lib as L
    import ivf_search
    eng, c = clstm
    x, tg = c['x'].cuda(), _tg(c)
    for kw in (dict(weights="mean"), dict(perturb="reverse"), dict(layer=5), dict(layer="cell0"), dict(channels=(3, 9)),
               dict(channels=(0, 0)), dict(channels=5)):
        with pytest.raises(L.IvfError):
            eng.scorecam(x, tg, **{**dict(layer=0), **kw})
    with pytest.raises(L.IvfError):
        eng.scorecam(x, tg[:1], layer=0)                             # one target for two clips
    with pytest.raises(L.IvfError):
        ivf_search.MaskSearch(eng, do_scorecam=True, scorecam_weights="mean")
    ivf_search.MaskSearch(eng, scorecam_weights="mean")              # off: read only when on
    # the C entry: null pointers and a bad grid come back as error codes, nothing is written
    lib = L.lib()
    planes = eng.scorecam_planes(x, 0)
    F = planes["F"]
    nc, gt, gh, gw = F.shape[1:]
    _, _, _, AH, AW = eng._st_axes((gh, gw), 1.0)
    sc = torch.full((2, nc + 1), -12345.0, device='cuda')
    tgt = torch.as_tensor(tg, dtype=torch.int32, device='cuda')
    fn = lib.ivf_clstm_scorecam_scores
    a = [eng._h, L.ptr(x), 2, L.ptr(tgt), L.ptr(AH), L.ptr(AW), gt, gh, gw, L.ptr(F), nc, 0, L.ptr(sc), L.stream()]
    for i, v in ((1, None), (3, None), (4, None), (9, None), (12, None), (2, 0), (10, 0), (11, 2), (6, gt + 1), (7, 33)):
        bad = list(a)
        bad[i] = v
        assert fn(*bad) == -1, i
    torch.cuda.synchronize()
    assert bool((sc == -12345.0).all())
    # the TF-style plan has no Score-CAM entry and refuses
    tf = ivf_engine.TFCLSTMEngine(5, (1, 8, 30, 40), units=(4,), kernel=(3, 5), stride=2, padding="valid", max_batch=1)
    assert not hasattr(lib, "ivf_tfclstm_scorecam_scores")
    with pytest.raises(L.IvfError):
        tf.scorecam(torch.zeros(1, 1, 8, 30, 40, device='cuda'), [0])
