"""Exhaustive one-blob temporal mask search (maskType 'combi') on the GPU: the score grids of ivf_*_blob_scores against
the reference's own mask.py + models (tests/golden/blob.npz, make_golden_blob.py) and against search.npz, staging
as an exact frame gather, chunking, the ConvLSTM's two recurrence paths, the device selection, and the drop-in
drivers' records."""
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import note, rel_err_elem

pytestmark = pytest.mark.gpu

EXACT = ("fp32", "bf16x6")
FLOOR = 1e-6          # scores are probabilities (softmax heads): every entry against its own magnitude


def _i3d(math, max_batch, kth=False):
    import ivf_engine
    import ivf_recipe as R
    if kth:
        eng = ivf_engine.I3DEngine(6, (3, 32, 120, 160), max_batch=max_batch, head_hw=(4, 5), head_time_base=4,
                                   softmax=True, math=math)
        eng.load_state_dict(R.i3d_state_dict(num_classes=6, tag='i3d_kth'))
    else:
        eng = ivf_engine.I3DEngine(174, (3, 16, 224, 224), max_batch=max_batch, softmax=True, math=math)
        eng.load_state_dict(R.i3d_state_dict(num_classes=174))
    return eng


def _clstm(max_batch):
    import ivf_engine
    import ivf_recipe as R
    eng = ivf_engine.CLSTMEngine(6, (1, 32, 120, 160), max_batch=max_batch, hidden=4, layers=2, kernel=5, stride=2,
                                 softmax=True)
    eng.load_state_dict(R.clstm_state_dict(channels=1, tag='clstm1'))
    return eng


@pytest.fixture(scope="module", params=["fp32", "bf16x3", "bf16x6"])
def s16(request):
    return _i3d(request.param, 32)


@pytest.fixture(scope="module", params=["fp32", "bf16x3", "bf16x6"])
def k32(request):
    return _i3d(request.param, 32, kth=True)


@pytest.fixture(scope="module")
def c1():
    return _clstm(32)


def _x(tag):
    import ivf_recipe as R
    if tag == "s16":
        return torch.from_numpy(R.clip(21))[None].cuda()
    if tag == "k32":
        return torch.from_numpy(R.clip(23, 3, 32, 120, 160))[None].cuda()
    return (torch.from_numpy(R.clip(3, 1, 32, 120, 160) / 255.0)[None]).float().cuda()


def _gate(math):
    return 1e-5 if math in EXACT else 1e-3


def _grid_vs_reference(eng, tag, mode, g):
    x = _x(tag)
    t = int(g[f'{tag}_target'])
    assert int(torch.argmax(eng.forward(x)[0])) == t
    ml = int(g[f'{tag}_max_len'])
    got = eng.blob_scores(x, [t], ml, mode)[0].cpu().numpy()
    ref = g[f'{tag}_{mode}_scores']
    assert got.shape == ref.shape
    e = rel_err_elem(got, ref, FLOOR)
    note(f"blob grid {tag} {mode} {getattr(eng, 'math', 'clstm')}: {ref.size} entries, elementwise rel {e:.2e}, "
         f"max abs {np.max(np.abs(got - ref)):.2e}")
    assert e < 1e-3
    return x, t, got


# ------------------------------------------------------------------ 1. grids vs the reference
@pytest.mark.parametrize("mode", ["freeze", "reverse"])
def test_s16_grid_vs_reference(s16, mode, golden):
    _grid_vs_reference(s16, "s16", mode, golden('blob'))


def test_k32_grid_vs_reference(k32, golden):
    _grid_vs_reference(k32, "k32", "freeze", golden('blob'))


@pytest.mark.parametrize("mode", ["freeze", "reverse"])
def test_clstm_grid_vs_reference(c1, mode, golden):
    _grid_vs_reference(c1, "c1", mode, golden('blob'))


# ------------------------------------------------------------------ 2. grid vs search.npz (no new data)
def test_s16_grid_vs_search_fixture(s16, golden):
    import ivf_search
    g = golden('search')
    x = _x("s16")
    grid = s16.blob_scores(x, [int(g['s16_target'])], None, "freeze")[0].cpu().numpy()
    k = ivf_search.blob_index(torch.tensor([[0, 16]] + [[i, 16 - 2 * i] for i in range(1, len(g['s16_central']) + 1)]),
                              16).tolist()
    assert abs(grid[k[0]] - float(g['s16_full'])) < 1e-3 * float(g['s16_full'])       # the fully frozen clip
    for i, ref in enumerate(g['s16_central'], start=1):                                  # central mask i
        assert abs(grid[k[i]] - float(ref)) < 1e-3 * float(ref)


# ------------------------------------------------------------------ 3. staging is a frame gather
@pytest.mark.parametrize("mode", ["freeze", "reverse"])
def test_staging_equals_perturbed_forward(s16, mode):
    import ivf_search
    x = _x("s16")
    t = int(torch.argmax(s16.forward(x)[0]))
    grid = s16.blob_scores(x, [t], None, mode)[0]
    cands = ivf_search.blob_candidates(16)
    masks = ivf_search.blob_masks(cands.cuda(), 16)
    n = cands.shape[0]
    # the same batch composition as the grid's chunks: the first full chunk and the 8-row tail -> bit-exact
    for first, cnt in ((0, 32), (128, n - 128)):
        p = s16.perturbed_forward(x.expand(cnt, -1, -1, -1, -1).contiguous(), masks[first:first + cnt], mode)[:, t]
        assert torch.equal(p, grid[first:first + cnt]), (mode, first)
    # a scattered sample in a batch of its own: the kernels may differ with the batch size
    ks = [0, 5, 17, 40, 77, 100, 131, 135]
    p = s16.perturbed_forward(x.expand(len(ks), -1, -1, -1, -1).contiguous(), masks[ks], mode)[:, t]
    e = rel_err_elem(p.cpu().numpy(), grid[ks].cpu().numpy(), FLOOR)
    note(f"blob staging vs perturbed_forward {mode} {s16.math}: other batch composition {e:.2e}")
    assert e < _gate(s16.math)


# ------------------------------------------------------------------ 4. chunking and rows are independent
def test_chunking_and_rows_independent(s16):
    import ivf_recipe as R
    x = _x("s16")
    t = int(torch.argmax(s16.forward(x)[0]))
    full = s16.blob_scores(x, [t], None, "freeze")[0].cpu().numpy()
    small = _i3d(s16.math, 7)
    g7 = small.blob_scores(x, [t], None, "freeze")[0].cpu().numpy()
    del small
    e7 = rel_err_elem(g7, full, FLOOR)
    # clip 1 of a two-clip call with another target == a one-clip call
    x2 = torch.cat([x, torch.from_numpy(R.clip(7))[None].cuda()])
    two = s16.blob_scores(x2, [t, 3], None, "freeze").cpu().numpy()
    one = s16.blob_scores(x2[1:], [3], None, "freeze")[0].cpu().numpy()
    e2 = rel_err_elem(two[1], one, FLOOR)
    e0 = rel_err_elem(two[0], full, FLOOR)
    # max_len = 8 is the prefix of the full grid
    g8 = s16.blob_scores(x, [t], 8, "freeze")[0].cpu().numpy()
    assert g8.shape == (8 * 17 - 36,)
    e8 = rel_err_elem(g8, full[:g8.size], FLOOR)
    note(f"blob chunking {s16.math}: B7 vs B32 {e7:.2e}, two-clip rows {e0:.2e} / {e2:.2e}, max_len 8 prefix {e8:.2e}")
    for e in (e7, e2, e0, e8):
        assert e < _gate(s16.math)


def test_blob_scores_refuses_bad_arguments(s16):
    import ivf_lib as L
    x = _x("s16")
    for ml in (0, 17):
        with pytest.raises(L.IvfError):
            s16.blob_scores(x, [0], ml)
    with pytest.raises(UnboundLocalError):
        s16.blob_scores(x, [0], None, "random")
    with pytest.raises(L.IvfError):
        s16.blob_scores(x, [0, 1])
    with pytest.raises(L.IvfError):
        s16.blob_scores(x[:, :, :8], [0])


# ------------------------------------------------------------------ 5. ConvLSTM: both recurrence paths
def test_clstm_persistent_and_step_paths_agree(c1):
    x = _x("c1")
    t = int(torch.argmax(c1.forward(x)[0]))
    g32 = c1.blob_scores(x, [t], None, "freeze")[0].cpu().numpy()     # chunks of 32: step kernels
    big = _clstm(64)
    g64 = big.blob_scores(x, [t], None, "freeze")[0].cpu().numpy()    # chunks of 64: persistent recurrence
    del big
    e = rel_err_elem(g64, g32, FLOOR)
    note(f"blob clstm grid, persistent (B64) vs step kernels (B32): {e:.2e}")
    assert e < 1e-5


# ------------------------------------------------------------------ 6. selection
def _selection_case(eng, tag, mode, g):
    import ivf_search
    x, t, got = _grid_vs_reference(eng, tag, mode, g)
    ref = g[f'{tag}_{mode}_scores'].astype(np.float64)
    err = float(np.max(np.abs(got - ref)))
    T = x.shape[2]
    ml = int(g[f'{tag}_max_len'])
    lam1, lam2 = (float(v) for v in g[f'{tag}_lam'])
    probs = eng.forward(x)
    orig = probs[:, t]
    full = eng.perturbed_forward(x, torch.ones(1, T, device='cuda'), "freeze")[:, t]
    sel = ivf_search.blob_select(torch.from_numpy(got)[None].cuda(), orig, full, T, ml, lam1, lam2, 0.9,
                                 want_obj=True)
    cands = [tuple(c) for c in ivf_search.blob_candidates(T, ml).tolist()]
    J = g[f'{tag}_{mode}_J'].astype(np.float64)
    best = tuple(sel["best"][0].tolist())
    order = np.argsort(J, kind='stable')
    gap = J[order[1]] - J[order[0]]
    if gap > 10 * err:
        assert best == tuple(g[f'{tag}_{mode}_best'])
    else:
        assert J[cands.index(best)] - J[order[0]] <= 2 * err
    assert abs(float(sel["objective"][0]) - float(sel["obj"][0, cands.index(best)])) == 0
    # J on the device = the reference's fp32 J up to the score error
    assert float(np.max(np.abs(sel["obj"][0].cpu().numpy() - J))) <= err + 1e-6
    # minimal sufficient blob: exact unless a ratio sits within the error of a decision
    o, f = float(g[f'{tag}_orig']), float(g[f'{tag}_full'])
    r = (o - ref) / (o - f)
    eps_r = 10 * (err + abs(float(orig) - o) + abs(float(full) - f)) * (2 + np.max(np.abs(r))) / abs(o - f)
    mref = tuple(g[f'{tag}_{mode}_minimal'])
    mgot = tuple(sel["minimal"][0].tolist())
    note(f"blob select {tag} {mode}: best {best} (ref {tuple(g[f'{tag}_{mode}_best'])}, gap {gap:.2e}, err {err:.2e}); "
         f"minimal {mgot} (ref {mref}, eps_r {eps_r:.2e})")
    if mgot != mref:
        near = np.abs(r - 0.9) <= eps_r
        close = mgot in cands and mref in cands and abs(r[cands.index(mgot)] - r[cands.index(mref)]) <= eps_r
        assert near.any() or close, (mgot, mref)


@pytest.mark.parametrize("mode", ["freeze", "reverse"])
def test_s16_selection(s16, mode, golden):
    _selection_case(s16, "s16", mode, golden('blob'))


def test_k32_selection(k32, golden):
    _selection_case(k32, "k32", "freeze", golden('blob'))


@pytest.mark.parametrize("mode", ["freeze", "reverse"])
def test_clstm_selection(c1, mode, golden):
    _selection_case(c1, "c1", mode, golden('blob'))


def test_selection_tie_rule_and_degenerate_rows():
    import ivf_search
    T, n = 8, 36
    cands = [tuple(c) for c in ivf_search.blob_candidates(T).tolist()]
    s = torch.ones(4, n)
    # row 0: exact ties at the minimum between (3,2), (5,2) and (1,3); (0,1) is NaN and skipped
    for c in ((3, 2), (5, 2), (1, 3)):
        s[0, cands.index(c)] = 0.2
    s[0, cands.index((0, 1))] = float("nan")
    # row 1: every score equal -> the first candidate, (0,1)
    s[1] = 0.5
    # row 2: no candidate reaches the threshold
    s[2] = 0.9
    # row 3: all NaN
    s[3] = float("nan")
    orig = torch.ones(4)
    full = torch.zeros(4)
    sel = ivf_search.blob_select(s.cuda(), orig.cuda(), full.cuda(), T, None, 0.0, 0.0, 0.8)
    best = [tuple(r) for r in sel["best"].tolist()]
    minimal = [tuple(r) for r in sel["minimal"].tolist()]
    assert best[0] == (3, 2) and minimal[0] == (3, 2)      # r = 0.8 at (3,2), (5,2), (1,3): smallest L, then a
    assert best[1] == (0, 1) and minimal[1] == (-1, -1)    # r = 0.5 < 0.8
    assert best[2] == (0, 1) and minimal[2] == (-1, -1)
    assert best[3] == (-1, -1) and minimal[3] == (-1, -1) and np.isnan(float(sel["objective"][3]))
    assert float(sel["objective"][1]) == 0.5
    # ties on r: the largest r within the smallest L, then the smallest a
    s2 = torch.full((1, n), 0.5)
    s2[0, cands.index((6, 1))] = 0.1
    s2[0, cands.index((2, 1))] = 0.1
    s2[0, cands.index((4, 1))] = 0.15
    sel = ivf_search.blob_select(s2.cuda(), torch.ones(1).cuda(), torch.zeros(1).cuda(), T, None, 0.01, 0.02, 0.8)
    assert tuple(sel["minimal"][0].tolist()) == (2, 1)


def test_tv_term_bit_identical_to_search_regulariser():
    """J - s at a binary mask is the search loop's own regulariser (ivf_mask_reg at a saturated sigmoid), bit for
    bit, for every blob at T = 16 and T = 32."""
    import ivf_lib as L
    import ivf_search
    for T in (16, 32):
        cands = ivf_search.blob_candidates(T)
        n = cands.shape[0]
        masks = ivf_search.blob_masks(cands.cuda(), T)
        sel = ivf_search.blob_select(torch.zeros(1, n, device='cuda'), torch.ones(1, device='cuda'),
                                     torch.zeros(1, device='cuda'), T, None, 0.01, 0.02, 0.9, want_obj=True)
        raw = (masks * 200.0 - 100.0).contiguous()        # sigmoid(+-100) is exactly 1 / 0 in fp32
        sig = torch.empty_like(raw)
        terms = torch.empty(n, 2, device='cuda')
        dreg = torch.empty_like(raw)
        L.check(L.lib().ivf_mask_reg(L.ptr(raw), n, T, 0.01, 0.02, L.ptr(sig), L.ptr(terms), L.ptr(dreg), L.stream()))
        assert torch.equal(sig, masks)
        assert torch.equal(sel["obj"][0], terms[:, 0] + terms[:, 1])


# ------------------------------------------------------------------ 7. the drop-in drivers
REF_KEYS = {'true_class', 'pred_class', 'video_id', 'time_mask', 'original_score_guess', 'original_score_true',
            'freeze_score', 'reverse_score'}


def _check_combi_records(net, tm, xs, ml, T, sub):
    import ivf_search
    assert len(tm) == xs.shape[0]
    eng = net._engine_for(xs)
    masks = []
    for j, rec in enumerate(tm):
        assert set(rec) == REF_KEYS | {'blob_start', 'blob_length', 'blob_scores'}
        a, ln = rec['blob_start'], rec['blob_length']
        assert 1 <= ln <= ml and 0 <= a <= T - ln
        want = np.zeros(T, np.float32)
        want[a:a + ln] = 1
        assert np.array_equal(rec['time_mask'], want)
        assert rec['blob_scores'].shape == (ml * (T + 1) - ml * (ml + 1) // 2,)
        k = int(ivf_search.blob_index(torch.tensor([[a, ln]]), T)[0])
        assert rec['freeze_score'] == float(rec['blob_scores'][k])
        masks.append(want)
    rev = eng.perturbed_forward(xs, torch.from_numpy(np.stack(masks)).cuda(), "reverse")
    for j, rec in enumerate(tm):
        assert rec['reverse_score'] == float(rev[j, rec['pred_class']])
    files = [os.path.basename(str(p)) for p in sub.rglob("*.txt")]
    for rec in tm:
        assert "ClassScoreFreezecase" + str(rec['video_id']) + ".txt" in files
        assert "ClassScoreReversecase" + str(rec['video_id']) + ".txt" in files


def test_find_masks_combi_smth(tmp_path, monkeypatch):
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    import ivf_recipe as R
    from models import I3D_doubled
    monkeypatch.chdir(tmp_path)
    m = I3D_doubled.Model(174, last_stride=1, stride_mod_layers="", softMax=1)
    m.load_state_dict({"module." + k: v for k, v in R.to_torch(R.i3d_state_dict(num_classes=174)).items()})
    m = m.cuda().eval()
    loader = ivf_find_masks.SyntheticLoader(2, 2, (3, 16, 224, 224), 174, first_id=40)
    hp = {"batch_size": 2, "gradCamType": "guessed"}
    drv.find_masks(loader, m, hp, 0.01, 0.02, 5, maskType="combi", temporalMaskType="freeze", classOI=None,
                   verbose=False, maxMaskLength=4, doGradCam=False, runTempMask=True)
    tm = pickle.load(open(tmp_path / "results" / "allTimeMaskResults_run0_None_.p", "rb"))
    gc = pickle.load(open(tmp_path / "results" / "allGradCamResults_run0_None_.p", "rb"))
    assert gc == []
    xs = next(iter(loader))[0].float().cuda()
    _check_combi_records(m, tm, xs, 4, 16, tmp_path / "cam_saved_images")
    assert m._engine_for(xs).max_batch >= 32          # the candidates of the loader batch fill a 32-row plan


def test_find_masks_combi_kth_clstm(tmp_path, monkeypatch):
    import FindMasksComparison_I3D_KTH as drv
    import ivf_find_masks
    import ivf_recipe as R
    from models import CLSTM_4
    monkeypatch.chdir(tmp_path)
    m = CLSTM_4.Model(num_classes=6, nb_lstm_units=4, channels=3, conv_kernel_size=(5, 5), lstm_layers=2,
                      step=32, image_size=(160, 120), conv_stride=2, effective_step=[7, 15, 23, 31])
    m.load_state_dict(R.to_torch(R.clstm_state_dict(channels=3, tag='clstm3')))
    m = m.cuda().eval()
    loader = ivf_find_masks.SyntheticLoader(2, 2, (3, 32, 120, 160), 6, first_id=7)
    cfg = {"batch_size": 2, "gradCamType": "guessed"}
    masks = drv.find_masks(loader, m, cfg, 0.02, 0.04, 4, 1, "combi", "reverse", classOI=None, verbose=False,
                           maxMaskLength=6, doGradCam=False, runTempMask=True)
    assert len(masks) == 2
    tm = pickle.load(open(tmp_path / "results" / "I3d_KTH_allTimeMaskResults_original_run0.p", "rb"))
    xs = next(iter(loader))[0].float().cuda()
    # reverse is the loop-type perturbation here: freeze_score is the reverse score of the best blob
    for rec in tm:
        assert rec['freeze_score'] == rec['reverse_score']
    _check_combi_records(m, tm, xs, 6, 32, tmp_path / "cam_saved_images")
