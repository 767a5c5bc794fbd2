"""Exhaustive one-box spatio-temporal mask search (maskType 'stcombi') on the GPU: the staging kernel
against ivf_stmask_expand_fwd + ivf_stfreeze_fwd on the explicit binary S (equality), its reduction to ivf_blob_stage on
a 1 x 1 grid, the score grids against st_perturbed_forward and against tests/golden/box.npz (make_golden_box.py: the
reference's I3D model under the torch restatement of expand and per-pixel freeze), the device selection and drop map
against tests/box_refs.py, and the drop-in drivers' records.  tests/test_box_refs_host.py proves the references on the
CPU."""
import os
import pickle

import numpy as np
import pytest
import torch

import box_refs as B
import stmask_refs as SR
from conftest import note, rel_err_elem
from test_gpu_leaf_kernels import bits, guarded, untouched

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00ABC
FLOOR = 1e-6          # scores are probabilities (softmax heads): every entry against its own magnitude (test_gpu_blob.py)
EXACT = ("fp32", "bf16x6")


def _gate(math):
    """test_gpu_blob.py's gate for the same rows in another batch composition"""
    return 1e-5 if math in EXACT else 1e-3


# ---------------------------------------------------------------------------------------------------- A. staging
def _stage(xd, AHd, AWd, dims, first, count, cpad):
    import ivf_lib as L
    b, C, T, H, W, (gh, gw), ml, (mh, mw) = dims
    buf, p = guarded((count, C, T, H * W) if cpad == 0 else (count, T, H * W, 4))
    bits(p).fill_(NAN_BITS)
    L.check(L.lib().ivf_box_stage(L.ptr(xd), b, C, T, H, W, L.ptr(AHd), L.ptr(AWd), gh, gw, ml, mh, mw, first, count, L.ptr(p),
                                  cpad, L.stream()))
    torch.cuda.synchronize()
    assert untouched(buf), f"box_stage out_cpad={cpad}: a sentinel row was written"
    assert not bool(torch.isnan(p).any()), f"box_stage out_cpad={cpad}: an element was never written"
    return p


def _pair(xd, AHd, AWd, dims, tab, first, count, cpad):
    """the same rows by ivf_stmask_expand_fwd + ivf_stfreeze_fwd on the explicit S of each candidate"""
    import ivf_lib as L
    b, C, T, H, W, (gh, gw), ml, mb = dims
    n = len(tab)
    rows = np.arange(first, first + count)
    S = torch.stack([B.box_S(tab[g % n], T, (gh, gw)) for g in rows]).cuda().contiguous()
    xr = xd[torch.from_numpy(rows // n).cuda()].contiguous()
    M = torch.empty(count, T, H, W, device='cuda')
    L.check(L.lib().ivf_stmask_expand_fwd(L.ptr(S), L.ptr(AHd), L.ptr(AWd), L.ptr(M), count, T, gh, gw, H, W, L.stream()))
    p = torch.empty((count, C, T, H * W) if cpad == 0 else (count, T, H * W, 4), device='cuda')
    L.check(L.lib().ivf_stfreeze_fwd(L.ptr(xr), L.ptr(M), L.ptr(p), count, C, T, H * W, cpad, L.stream()))
    torch.cuda.synchronize()
    return p


def _check_windows(C, T, sigma, ml, cpad, windows, H=12, W=20, grid=(3, 4), mb=(2, 3), b=2):
    gh, gw = grid
    dims = (b, C, T, H, W, grid, ml, mb)
    tab = B.box_table(T, grid, ml, mb)
    n = len(tab)
    xd = B.stage_inputs(b, C, T, H, W).cuda()
    AHd, AWd = SR.axis_weights(H, gh, sigma).cuda(), SR.axis_weights(W, gw, sigma).cuda()
    moved = 0
    for first, count in windows(n):
        assert 0 <= first and first + count <= b * n
        got = _stage(xd, AHd, AWd, dims, first, count, cpad)
        want = _pair(xd, AHd, AWd, dims, tab, first, count, cpad)
        assert torch.equal(got, want), f"rows [{first}, {first + count}) of {b * n}: not the bits of expand_fwd + stfreeze_fwd"
        if cpad == 4:
            assert torch.equal(bits(got[..., C:]), torch.zeros_like(bits(got[..., C:]))), "pad lane not +0.0"
        src = xd[torch.from_numpy(np.arange(first, first + count) // n).cuda()]
        flat = got if cpad == 0 else got[..., :C].permute(0, 3, 1, 2)
        moved += int((flat != src.reshape(count, C, T, H * W)).any(dim=(1, 2, 3)).sum())
    assert moved > 0, "no staged row differs from its clip: the comparison is vacuous"
    return n


@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("sigma", [0.0, 1.5])
@pytest.mark.parametrize("C", [1, 3])
def test_staging_is_expand_plus_freeze_on_the_explicit_mask(C, sigma, cpad):
    """A.  b = 2, T = 5, 12 x 20, grid 3 x 4, max_len 3, max_box (2, 3): windows that start mid-clip, cross the clip
    boundary and end on the last row, and the whole list in one call"""
    n = _check_windows(C, 5, sigma, 3, cpad, lambda n: [(37, 200), (n - 50, 120), (2 * n - 64, 64), (0, 2 * n)])
    assert n == 12 * 5 * 9


@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("T", [17, 40, 16, 32])
def test_staging_on_every_frame_count_path(T, cpad):
    """A, repeated with max_len 2 at T = 17 and T = 40 (the frame loop of the 16-byte kernel) and at T = 16 and T = 32
    (its pieces of 16 preloaded frames)"""
    _check_windows(3, T, 1.5, 2, cpad, lambda n: [(n // 2 + 3, 40), (n - 30, 70), (2 * n - 50, 50)])


# ---------------------------------------------------------------------------------------------------- B. 1 x 1 grid
@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("T", [5, 16])
def test_1x1_grid_reduces_to_blob_stage(T, cpad):
    """grid 1 x 1, sigma 0: A is all ones, M = 1 on the blob, the freeze returns P[u-1] exactly -- ivf_blob_stage(mode 0)
    row for row"""
    import ivf_lib as L
    b, C, H, W, ml = 2, 3, 12, 20, min(T, 6)
    xd = B.stage_inputs(b, C, T, H, W).cuda()
    AHd, AWd = SR.axis_weights(H, 1, 0.0).cuda(), SR.axis_weights(W, 1, 0.0).cuda()
    n = L.lib().ivf_blob_count(T, ml)
    assert L.lib().ivf_box_count(T, ml, 1, 1, 1, 1) == n
    got = _stage(xd, AHd, AWd, (b, C, T, H, W, (1, 1), ml, (1, 1)), 0, b * n, cpad)
    want = torch.empty_like(got)
    L.check(L.lib().ivf_blob_stage(L.ptr(xd), b, C, T, H * W, ml, 0, 0, b * n, L.ptr(want), cpad, L.stream()))
    torch.cuda.synchronize()
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------- plans
def _s16_x(clips=(21,)):
    import ivf_recipe as RC
    return torch.from_numpy(np.stack([RC.clip(c) for c in clips])).cuda()


@pytest.fixture(scope="module", params=["fp32", "bf16x3", "bf16x6"])
def s16(request):
    import ivf_engine
    import ivf_recipe as RC
    eng = ivf_engine.I3DEngine(174, (3, 16, 224, 224), max_batch=32, softmax=True, math=request.param)
    eng.load_state_dict(RC.i3d_state_dict(num_classes=174))
    return eng


@pytest.fixture(scope="module")
def s16_grid(s16):
    """the score grid both the fixture test and the selection test read: clip 21, grid 2 x 2, sigma 0, max_len 2, max_box
    (2, 2) -- 31 * 3 * 3 = 279 candidates"""
    x = _s16_x()
    probs = s16.forward(x)
    t = int(torch.argmax(probs[0]))
    scores = s16.box_scores(x, [t], (2, 2), 0.0, 2, (2, 2))
    full = s16.perturbed_forward(x, torch.ones(1, 16, device='cuda'), "freeze")[:, t]
    return x, t, probs[:, t].clone(), full, scores


@pytest.fixture(scope="module")
def clstm():
    """the ConvLSTM plan of clstm_refs case S2 (C 2, T 6, 24 x 32, two layers), as test_gpu_stmask.py builds it"""
    import ivf_engine
    c = SR.chain_case()
    case = c['case']
    eng = ivf_engine.CLSTMEngine(5, (case.C, case.T, case.H, case.W), max_batch=case.B, hidden=case.hid, layers=case.layers,
                                 kernel=case.k, stride=case.s, softmax=case.softmax, batch_norm=case.batch_norm)
    eng.load_state_dict(c['sd'])
    return eng, c


def _tg(c):
    return [int(v) for v in c['targets']]


def _chain(eng, x, targets, grid, sigma, ml, mb, math):
    """C.  box_scores == st_perturbed_forward of the explicit expanded masks in the same chunk composition (equality);
    the rows of clip 1 of a two-clip call start at another place of their chunk: the other-composition gate"""
    import ivf_search
    b, T = x.shape[0], x.shape[2]
    Bp = eng.max_batch
    scores = eng.box_scores(x, targets, grid, sigma, ml, mb)
    tab = ivf_search.box_candidates(T, grid, ml, mb)
    n = tab.shape[0]
    assert tuple(scores.shape) == (b, n)
    S = ivf_search.box_masks(tab.cuda(), T, grid)                    # [n,T,gh,gw]
    flat = scores.reshape(-1)
    tl = torch.as_tensor(targets, device='cuda').long()
    for first in range(0, b * n, Bp):
        rows = torch.arange(first, min(first + Bp, b * n), device='cuda')
        clip, k = rows // n, rows % n
        M = eng.st_expand(S[k].contiguous(), grid, sigma)
        p = eng.st_perturbed_forward(x[clip].contiguous(), M)[torch.arange(len(rows), device='cuda'), tl[clip]]
        assert torch.equal(p, flat[first:first + len(rows)]), f"chunk at row {first}"
    e = 0.0
    if b > 1:
        one = eng.box_scores(x[1:].contiguous(), list(targets[1:]), grid, sigma, ml, mb)
        assert n % Bp != 0
        e = rel_err_elem(scores[1:].cpu().numpy(), one.cpu().numpy(), FLOOR)
        assert e < _gate(math)
    return n, e


def test_i3d_grid_equals_st_perturbed_forward(s16):
    x = _s16_x((21, 7))
    targets = s16.argmax(s16.forward(x)).tolist()
    n, e = _chain(s16, x, targets, (2, 2), 0.0, 2, (1, 1), s16.math)
    assert n == 124
    note(f"box chain I3D {s16.math}: {2 * n} rows bit-equal to st_perturbed_forward; clip 1 at another chunk offset {e:.2e}")


def test_clstm_grid_equals_st_perturbed_forward(clstm):
    eng, c = clstm
    n, e = _chain(eng, c['x'].cuda(), _tg(c), SR.CHAIN_GRID, SR.CHAIN_SIGMA, 2, (2, 2), "fp32")
    assert n == 11 * 5 * 7
    note(f"box chain ConvLSTM S2: rows bit-equal to st_perturbed_forward; clip 1 at another chunk offset {e:.2e}")


# ---------------------------------------------------------------------------------------------------- D. golden
def test_s16_scores_vs_fixture(s16, s16_grid, golden):
    """the listed candidates of tests/golden/box.npz within 1e-3 relative, each against its own magnitude"""
    g = golden('box')
    x, t, orig, full, scores = s16_grid
    grid, ml, mb = tuple(int(v) for v in g['grid']), int(g['max_len']), tuple(int(v) for v in g['max_box'])
    assert (grid, ml, mb, float(g['sigma']), int(g['clip'])) == ((2, 2), 2, (2, 2), 0.0, 21)
    assert t == int(g['target'])                                   # integer output: bit-exact
    ks = [B.box_index(c, 16, grid, mb) for c in g['candidates']]
    got = scores[0, ks].cpu().numpy()
    e = rel_err_elem(got, g['scores'], FLOOR)
    note(f"box grid vs fixture {s16.math}: {len(ks)} candidates, elementwise rel {e:.2e}, orig {abs(float(orig[0]) - float(g['orig'])):.2e} abs")
    assert e < 1e-3
    assert abs(float(orig[0]) - float(g['orig'])) < 1e-3 * float(g['orig'])


# ---------------------------------------------------------------------------------------------------- E. selection
def _check_selection(scores, orig, full, T, grid, ml, mb, lams, threshold, what):
    import ivf_search
    sel = ivf_search.box_select(scores, orig, full, T, grid, ml, mb, lams[0], lams[1], lams[2], threshold, want_obj=True)
    tab = B.box_table(T, grid, ml, mb)
    s = scores.cpu().numpy()
    o, f = orig.cpu().numpy(), full.cpu().numpy()
    obj = sel["obj"].cpu().numpy()
    J64, bound = B.objective64(tab, s, T, grid, lams)
    ok = ~np.isnan(s)
    assert np.array_equal(np.isnan(obj), ~ok)
    err = np.abs(obj.astype(np.float64) - J64)
    assert bool((err[ok] <= bound[ok]).all()), f"{what}: J off by {float((err[ok] - bound[ok]).max()):.3e} beyond its bound"
    assert np.array_equal(bits(torch.from_numpy(obj)).numpy()[ok], bits(torch.from_numpy(B.objective32(tab, s, T, grid, lams))).numpy()[ok])
    best, minimal = B.select_rule(obj, s, o, f, tab, threshold)
    for r in range(s.shape[0]):
        for name, k, got in (("best", best[r], sel["best"][r]), ("minimal", minimal[r], sel["minimal"][r])):
            want = tuple(tab[k]) if k >= 0 else (-1,) * 6
            assert tuple(got.tolist()) == tuple(int(v) for v in want), f"{what} row {r} {name}"
        assert int(sel["index"][r]) == best[r]
        if best[r] >= 0:
            assert float(sel["objective"][r]) == float(obj[r, best[r]])
        else:
            assert np.isnan(float(sel["objective"][r]))
    worst = float((err[ok] / np.maximum(bound[ok], 1e-300)).max()) if ok.any() else 0.0
    return sel, best, minimal, worst


def test_selection_on_the_i3d_grid(s16, s16_grid):
    x, t, orig, full, scores = s16_grid
    sel, best, minimal, worst = _check_selection(scores, orig, full, 16, (2, 2), 2, (2, 2), (0.01, 0.02, 0.03), 0.05, "S16")
    note(f"box select S16 {s16.math}: best {tuple(sel['best'][0].tolist())} minimal {tuple(sel['minimal'][0].tolist())}, "
         f"J worst err/gate {worst:.3f}")


def test_selection_on_the_clstm_grid(clstm):
    eng, c = clstm
    x = c['x'].cuda()
    b, T = x.shape[0], x.shape[2]
    tg = torch.as_tensor(_tg(c), device='cuda').long()
    idx = torch.arange(b, device='cuda')
    orig = eng.forward(x)[idx, tg]
    full = eng.perturbed_forward(x, torch.ones(b, T, device='cuda'), "freeze")[idx, tg]
    scores = eng.box_scores(x, _tg(c), SR.CHAIN_GRID, SR.CHAIN_SIGMA, 2, (2, 2))
    sel, best, minimal, worst = _check_selection(scores, orig, full, T, SR.CHAIN_GRID, 2, (2, 2), (0.01, 0.02, 0.03), 0.3, "S2")
    note(f"box select ConvLSTM S2: best {sel['best'].tolist()} minimal {sel['minimal'].tolist()}, J worst err/gate {worst:.3f}")


def test_selection_tie_rules_and_degenerate_rows():
    T, grid, ml, mb = 4, (2, 3), 3, (2, 2)
    tab = B.box_table(T, grid, ml, mb)
    n = len(tab)
    k = lambda *c: B.box_index(c, T, grid, mb)
    s = torch.ones(6, n)
    # row 0: equal J at three candidates of equal volume and r (lam = 0) -> the smallest k, for best and for minimal
    ties = [k(2, 1, 1, 1, 2, 1), k(1, 1, 0, 1, 1, 1), k(3, 1, 0, 1, 0, 1)]
    s[0, ties] = 0.25
    # row 1: a larger box reaches a larger r, a unit box only just the threshold: minimal takes the smaller volume, and
    # within the unit boxes the larger r, whatever the order of k
    s[1] = 0.9
    s[1, k(0, 2, 0, 2, 0, 2)] = 0.0
    s[1, k(1, 1, 0, 1, 0, 1)] = 0.25
    s[1, k(2, 1, 1, 1, 1, 1)] = 0.125
    s[1, k(3, 1, 1, 1, 2, 1)] = 0.125
    # row 2: every score equal -> candidate 0; nothing reaches the threshold
    s[2] = 0.5
    # row 3: all NaN
    s[3] = float('nan')
    # row 4: the minimum sits behind NaN scores
    s[4] = 0.75
    s[4, :5] = float('nan')
    # row 5: as row 0 (the NaN column below must not disturb it)
    s[5] = s[0]
    s[:, 7] = float('nan')                                         # a NaN column
    orig, full = torch.ones(6), torch.zeros(6)
    sel, best, minimal, _ = _check_selection(s.cuda(), orig.cuda(), full.cuda(), T, grid, ml, mb, (0.0, 0.0, 0.0), 0.75, "constructed")
    assert best[0] == min(ties) and minimal[0] == min(ties) and best[5] == best[0]
    assert best[1] == k(0, 2, 0, 2, 0, 2) and minimal[1] == min(k(2, 1, 1, 1, 1, 1), k(3, 1, 1, 1, 2, 1))
    assert best[2] == 0 and minimal[2] == -1
    assert best[3] == -1 and minimal[3] == -1
    assert best[4] == 5 and minimal[4] == -1
    # with the regulariser on, the same rows still follow the rule, and J carries the closed-form terms
    _check_selection(s.cuda(), orig.cuda(), full.cuda(), T, grid, ml, mb, (0.01, 0.02, 0.03), 0.75, "constructed, lam > 0")


# ---------------------------------------------------------------------------------------------------- F. drop map
def test_drop_map():
    import ivf_search
    T, grid, ml, mb, b = 5, (3, 4), 3, (2, 3), 3
    tab = B.box_table(T, grid, ml, mb)
    n = len(tab)
    g = SR._gen('boxdrop')
    s = torch.rand(b, n, generator=g)
    orig = torch.tensor([0.9, 0.6, 0.3])
    sd, od = s.cuda(), orig.cuda()
    drop = ivf_search.box_drop(sd, od, T, grid, ml, mb)
    ref, bound, cnt = B.drop_ref(s.numpy(), orig.numpy(), tab, T, grid)
    assert int(cnt.min()) >= 1
    err = np.abs(drop.cpu().numpy().astype(np.float64) - ref)
    assert bool((err <= bound).all()), f"drop: worst {float((err - bound).max()):.3e} over"
    # rows of a b-clip call == one-clip calls, bit for bit
    for r in range(b):
        one = ivf_search.box_drop(sd[r:r + 1].contiguous(), od[r:r + 1].contiguous(), T, grid, ml, mb)
        assert torch.equal(bits(one), bits(drop[r:r + 1]))
    # a NaN score changes the cells it covers and no other
    kn = B.box_index((1, 2, 1, 2, 0, 3), T, grid, mb)
    s2 = s.clone()
    s2[1, kn] = float('nan')
    d2 = ivf_search.box_drop(s2.cuda(), od, T, grid, ml, mb)
    covered = torch.zeros(b, T, *grid, dtype=torch.bool)
    covered[1, 1:3, 1:3, 0:3] = True
    same = bits(d2).cpu() == bits(drop).cpu()
    assert bool(same[~covered].all()) and not bool(same[covered].any())
    ref2, bound2, cnt2 = B.drop_ref(s2.numpy(), orig.numpy(), tab, T, grid)
    assert np.array_equal(cnt - cnt2, covered.numpy().astype(np.float64))
    assert bool((np.abs(d2.cpu().numpy().astype(np.float64) - ref2) <= bound2).all())
    # all scores NaN: no candidate is left, the map says so
    assert bool(torch.isnan(ivf_search.box_drop(torch.full((1, n), float('nan'), device='cuda'), od[:1].contiguous(), T, grid, ml, mb)).all())
    note(f"box drop map {(b, T) + grid}: counts {int(cnt.min())}..{int(cnt.max())}, worst err/gate {float((err / bound).max()):.3f}")


# ---------------------------------------------------------------------------------------------------- G. drivers
REF_KEYS = {'true_class', 'pred_class', 'video_id', 'time_mask', 'original_score_guess', 'original_score_true',
            'freeze_score', 'reverse_score'}
BOX_KEYS = {'st_mask', 'box_start', 'box_length', 'box_rows', 'box_cols', 'box_drop'}


def _check_box_records(net, recs, xs, T, grid, ml, mb, sub):
    gh, gw = grid
    eng = net._engine_for(xs)
    assert eng.max_batch >= 32                       # the candidates of the loader batch fill a 32-row plan
    scores = eng.box_scores(xs, [r['pred_class'] for r in recs], grid, None, ml, mb).cpu().numpy()
    assert len(recs) == xs.shape[0]
    for j, r in enumerate(recs):
        assert set(r) == REF_KEYS | BOX_KEYS
        a, ln, (i0, bh), (j0, bw) = r['box_start'], r['box_length'], r['box_rows'], r['box_cols']
        assert 1 <= ln <= ml and 0 <= a <= T - ln and 1 <= bh <= mb[0] and 0 <= i0 <= gh - bh and 1 <= bw <= mb[1] and 0 <= j0 <= gw - bw
        want = B.box_S((a, ln, i0, bh, j0, bw), T, grid).numpy()
        assert r['st_mask'].dtype == np.float32 and np.array_equal(r['st_mask'], want)
        assert r['freeze_score'] == float(scores[j, B.box_index((a, ln, i0, bh, j0, bw), T, grid, mb)])
        mean = want.astype(np.float64).mean(axis=(1, 2))
        assert r['time_mask'].shape == (T,) and np.max(np.abs(r['time_mask'] - mean)) <= SR.gamma(gh + gw + 2) * max(mean.max(), 1e-30)
        assert r['box_drop'].shape == (T, gh, gw) and np.isfinite(r['box_drop']).all()
        assert np.isfinite(r['reverse_score'])
    files = [os.path.basename(str(p)) for p in sub.rglob("*.txt")]
    for r in recs:
        assert "ClassScoreFreezecase" + str(r['video_id']) + ".txt" in files
        assert "ClassScoreReversecase" + str(r['video_id']) + ".txt" in files


def test_find_masks_stcombi_smth(tmp_path, monkeypatch):
    """find_masks(maskType='stcombi') on I3D, two synthetic clips; maskType='central' does not see the new keyword: its
    records are byte-identical with and without it"""
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    import ivf_recipe as RC
    from models import I3D_doubled
    m = I3D_doubled.Model(174, last_stride=1, stride_mod_layers="", softMax=1)
    m.load_state_dict({"module." + k: v for k, v in RC.to_torch(RC.i3d_state_dict(num_classes=174)).items()})
    m = m.cuda().eval()
    monkeypatch.chdir(tmp_path)
    hp = {"batch_size": 2, "gradCamType": "guessed"}

    def run(mask_type, **kw):
        loader = ivf_find_masks.SyntheticLoader(2, 2, (3, 16, 224, 224), 174, first_id=40)
        drv.find_masks(loader, m, hp, 0.01, 0.02, 2, mask_type, "freeze", classOI=None, doGradCam=False, runTempMask=True,
                       verbose=False, **kw)
        return ivf_find_masks.find_masks_impl.last_results[0]

    run("stcombi", maxMaskLength=2, maskGrid=(2, 2), maxBox=(1, 2))
    recs = pickle.load(open(tmp_path / "results" / "allTimeMaskResults_run0_None_.p", "rb"))
    assert len(list((tmp_path / "cam_saved_images").rglob("mygif.gif"))) == 2          # strips from the expanded box
    xs = next(iter(ivf_find_masks.SyntheticLoader(2, 2, (3, 16, 224, 224), 174, first_id=40)))[0].float().cuda()
    _check_box_records(m, recs, xs, 16, (2, 2), 2, (1, 2), tmp_path / "cam_saved_images")
    plain = pickle.dumps(run("central"))
    assert set(pickle.loads(plain)[0]) == REF_KEYS
    assert pickle.dumps(run("central", maxBox=(1, 2), maxMaskLength=2, maskGrid=(2, 2))) == plain


def test_find_masks_stcombi_kth_clstm(tmp_path, monkeypatch):
    """the KTH driver with the ConvLSTM backbone, T = 32 at 120 x 160"""
    import FindMasksComparison_I3D_KTH as drv
    import ivf_find_masks
    import ivf_recipe as RC
    from models import CLSTM_4
    m = CLSTM_4.Model(num_classes=6, nb_lstm_units=4, channels=3, conv_kernel_size=(5, 5), lstm_layers=2,
                      step=32, image_size=(160, 120), conv_stride=2, effective_step=[7, 15, 23, 31])
    m.load_state_dict(RC.to_torch(RC.clstm_state_dict(channels=3, tag='clstm3')))
    m = m.cuda().eval()
    monkeypatch.chdir(tmp_path)
    cfg = {"batch_size": 2, "gradCamType": "guessed"}
    loader = ivf_find_masks.SyntheticLoader(2, 2, (3, 32, 120, 160), 6, first_id=7)
    masks = drv.find_masks(loader, m, cfg, 0.02, 0.04, 2, 1, "stcombi", "freeze", classOI=None, doGradCam=False,
                           runTempMask=True, verbose=False, maxMaskLength=2, maskGrid=(2, 3), maxBox=(2, 1))
    recs = pickle.load(open(tmp_path / "results" / "I3d_KTH_allTimeMaskResults_original_run0.p", "rb"))
    assert len(masks) == 2 and len(recs) == 2
    for r, mk in zip(recs, masks):
        assert np.array_equal(mk.cpu().numpy(), r['time_mask'])
    xs = next(iter(loader))[0].float().cuda()
    _check_box_records(m, recs, xs, 32, (2, 3), 2, (2, 1), tmp_path / "cam_saved_images")
    assert len(list((tmp_path / "cam_saved_images").rglob("case7pert3.png"))) == 1        # PNGs from the per-pixel freeze
    import ivf_lib as L
    with pytest.raises(L.IvfError):
        drv.find_masks(loader, m, cfg, 0.02, 0.04, 2, 1, "stcombi", "reverse", classOI=None, doGradCam=False,
                       runTempMask=True, verbose=False, maxMaskLength=2, maskGrid=(2, 3), maxBox=(2, 1))


# ---------------------------------------------------------------------------------------------------- H. refusals
def test_refusals(clstm):
    import ivf_engine
    import ivf_lib as L
    import ivf_search
    eng, c = clstm
    x = c['x'].cuda()
    b, C, T, H, W = x.shape
    tg = _tg(c)
    for grid, ml, mb in (((33, 4), 2, (1, 1)), ((3, 33), 2, (1, 1)), ((3, 4), 2, (4, 1)), ((3, 4), 2, (1, 5)), ((3, 4), T + 1, (1, 1)),
                         ((3, 4), 0, (1, 1)), ((3, 4), 2, (0, 1))):
        with pytest.raises(L.IvfError):
            eng.box_scores(x, tg, grid, 1.0, ml, mb)
        with pytest.raises(L.IvfError):
            ivf_search.box_select(torch.zeros(1, 4, device='cuda'), torch.ones(1, device='cuda'), torch.zeros(1, device='cuda'), T, grid, ml, mb)
        with pytest.raises(L.IvfError):
            ivf_search.box_drop(torch.zeros(1, 4, device='cuda'), torch.ones(1, device='cuda'), T, grid, ml, mb)
    with pytest.raises(L.IvfError):
        eng.box_scores(x, tg[:1], (3, 4), 1.0, 2, (1, 1))                       # one target for two clips
    with pytest.raises(L.IvfError):
        eng.box_scores(x[:, :, :4], tg, (3, 4), 1.0, 2, (1, 1))                 # not the plan's geometry
    # the C entries: null pointers and rows outside the list come back as error codes, nothing is written
    lib = L.lib()
    _, _, _, AH, AW = eng._st_axes((3, 4), 1.0)
    buf, p = guarded((2, C, T, H * W))
    n = lib.ivf_box_count(T, 2, 3, 4, 1, 1)
    args = lambda xs, ah, aw, first, count, pp, cpad: (L.ptr(xs), b, C, T, H, W, L.ptr(ah), L.ptr(aw), 3, 4, 2, 1, 1, first, count, L.ptr(pp), cpad, L.stream())
    assert lib.ivf_box_stage(*args(None, AH, AW, 0, 2, p, 0)) == -1 and b"box_stage" in lib.ivf_last_error()
    assert lib.ivf_box_stage(*args(x, None, AW, 0, 2, p, 0)) == -1
    assert lib.ivf_box_stage(*args(x, AH, None, 0, 2, p, 0)) == -1
    assert lib.ivf_box_stage(*args(x, AH, AW, 0, 2, None, 0)) == -1
    assert lib.ivf_box_stage(*args(x, AH, AW, b * n - 1, 2, p, 0)) == -1
    assert lib.ivf_box_stage(*args(x, AH, AW, -1, 2, p, 0)) == -1
    assert lib.ivf_box_stage(*args(x, AH, AW, 0, 0, p, 0)) == -1
    assert lib.ivf_box_stage(*args(x, AH, AW, 0, 2, p, 8)) == -1                  # layouts 0 and 4 only
    sc = torch.empty(b, n, device='cuda')
    tgt = torch.as_tensor(tg, dtype=torch.int32, device='cuda')
    fn = lib.ivf_clstm_box_scores
    assert fn(eng._h, None, b, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 4, 2, 1, 1, L.ptr(sc), L.stream()) == -1
    assert fn(eng._h, L.ptr(x), b, L.ptr(tgt), None, L.ptr(AW), 3, 4, 2, 1, 1, L.ptr(sc), L.stream()) == -1
    assert fn(eng._h, L.ptr(x), b, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 4, 2, 1, 1, None, L.stream()) == -1
    assert fn(eng._h, L.ptr(x), 0, L.ptr(tgt), L.ptr(AH), L.ptr(AW), 3, 4, 2, 1, 1, L.ptr(sc), L.stream()) == -1
    torch.cuda.synchronize()
    assert untouched(buf) and bool((p == -12345.0).all())
    # the TF-style plan has no spatio-temporal entries
    tf = ivf_engine.TFCLSTMEngine(5, (1, 8, 30, 40), units=(4,), kernel=(3, 5), stride=2, padding="valid", max_batch=1)
    assert not hasattr(lib, "ivf_tfclstm_box_scores")
    with pytest.raises(L.IvfError):
        tf.box_scores(torch.zeros(1, 1, 8, 30, 40, device='cuda'), [0], (2, 2), 0.0, 2, (1, 1))
    with pytest.raises(L.IvfError):
        ivf_search.MaskSearch(eng, mask_mode="stcombi", mask_type="reverse")
