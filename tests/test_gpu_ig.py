"""Integrated Gradients (csrc/ig_ops.hip) on the GPU: the three kernels against the fp64 references and
bounds of tests/ig_refs.py (test_ig_refs_host.py proves those on the CPU, on the same inputs), the whole method through
the ConvLSTM plan against torch fp64 autograd, the driver against its pieces, the I3D plan against the fixture
tests/golden/ig.npz (torch autograd on the reference's own model), and the Python surfaces.  Figures are written with
note() before anything is asserted."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

import clstm_refs as CR
import ig_refs as R
from conftest import note, rel_err
from leaf_refs import U, sum_bound

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _lib():
    import ivf_lib as L
    return L, L.lib()


# ---------------------------------------------------------------------------------------------------- stage
@pytest.mark.parametrize("layout", R.LAYOUTS, ids=["ncthw", "cl4"])
@pytest.mark.parametrize("kind", list(R.KINDS.values()), ids=list(R.KINDS))
def test_stage_matches_fp64(kind, layout):
    """Every shape of the table, every window: each element within gamma(3) max(|x|, |x0|) of fp64, bit-exact where
    x == x0 and at alpha == 0, pad lanes +0.0, nothing written outside the window's rows"""
    L, lib = _lib()
    worst, runs = 0.0, 0
    for shape in R.STAGE_SHAPES:
        B, C, T, HW, K = shape
        x, base, value = R.stage_inputs(shape, kind)
        x0 = R.baseline(x, kind, base, value)
        alpha = R.kernel_alpha(K)
        ref = R.stage_ref(x, x0, alpha).reshape(B * K, C, T, HW)
        bound = np.broadcast_to(R.stage_bound(x, x0), (B, K, C, T, HW)).reshape(B * K, C, T, HW)
        x0rows = np.broadcast_to(x0[:, None], (B, K, C, T, HW)).reshape(B * K, C, T, HW)
        same = np.broadcast_to((x == x0)[:, None], (B, K, C, T, HW)).reshape(B * K, C, T, HW)
        xd, bd, ad = _dev(x), _dev(base), _dev(alpha)
        row = C * T * HW if layout == 0 else T * HW * 4
        for first, count in R.windows(B, K):
            buf = torch.full(((count + 2) * row,), float("nan"), device="cuda")
            out = ctypes.c_void_p(buf.data_ptr() + row * 4)
            L.check(lib.ivf_ig_stage(L.ptr(xd), kind, L.ptr(bd), value, L.ptr(ad), B, C, T, HW, K, first, count, out,
                                     layout, L.stream()))
            h = buf.cpu().numpy()
            assert np.isnan(h[:row]).all() and np.isnan(h[-row:]).all(), (shape, first, count)
            body = h[row:-row].reshape((count, C, T, HW) if layout == 0 else (count, T, HW, 4))
            rows, pads = R.from_layout(body, layout, C)
            if pads is not None:
                assert not _bits(pads).any(), (shape, first, count)          # +0.0, bit for bit
            sl = slice(first, first + count)
            err = np.abs(rows.astype(F64) - ref[sl])
            assert not np.isnan(rows).any() and np.all(err <= bound[sl]), (shape, first, count)
            worst = max(worst, float(np.max(err / np.maximum(bound[sl], 1e-300))))
            assert _same_bits(rows[same[sl]], x0rows[sl][same[sl]]), (shape, first, count)
            for j in range(count):
                if alpha[(first + j) % K] == 0:
                    assert _same_bits(rows[j], x0rows[first + j]), (shape, first, count, j)
            runs += 1
    note(f"ig stage kind {kind} layout {layout}: {runs} windows, worst {worst:.2f} of the gamma(3) bound")


# ---------------------------------------------------------------------------------------------------- accumulate
def _accumulate(L, lib, rows, w, K, wins, b, layout):
    """Gsum [b,C,T,HW] after the windows `wins` of the row list `rows` [b*K,C,T,HW]; din has NaN pad lanes"""
    _, C, T, HW = rows.shape
    G = torch.zeros(b, C, T, HW, device="cuda")
    wd = _dev(w)
    for first, count in wins:
        din = _dev(R.to_layout(rows[first:first + count], layout, pad=np.nan))
        L.check(lib.ivf_ig_accumulate(L.ptr(din), layout, L.ptr(wd), K, first, count, L.ptr(G), b, C, T, HW, L.stream()))
    return G.cpu().numpy()


@pytest.mark.parametrize("layout", R.LAYOUTS, ids=["ncthw", "cl4"])
def test_accumulate_matches_fp64_and_is_window_invariant(layout):
    L, lib = _lib()
    for shape in R.ACC_SHAPES:
        B, C, T, HW, K = shape
        din, w = R.acc_inputs(shape)
        rows = din.reshape(B * K, C, T, HW)
        n = B * K
        g1 = _accumulate(L, lib, rows, w, K, [(0, n)], B, layout)
        ref, bound = R.gsum_ref(din, w)
        err = np.abs(g1.astype(F64) - ref)
        assert not np.isnan(g1).any() and np.all(err <= bound), shape
        note(f"ig accumulate {shape} layout {layout}: worst {float(np.max(err / bound)):.2f} of gamma(K+1) sum|w g|")
        splits = []
        if n >= 2:
            splits.append([(0, n // 2), (n // 2, n - n // 2)])
        if n >= 3:
            splits.append([(0, 1), (1, n - 2), (n - 1, 1)])              # cuts inside clips, a window over several
        for wins in splits:
            assert _same_bits(_accumulate(L, lib, rows, w, K, wins, B, layout), g1), (shape, wins)
        for r in range(B):                                              # batched rows == one-clip calls
            solo = _accumulate(L, lib, din[r], w, K, [(0, K)], 1, layout)
            assert _same_bits(solo[0], g1[r]), (shape, r)


# ---------------------------------------------------------------------------------------------------- finish
def _finish(L, lib, x, kind, base, value, gsum):
    B, C, T, HW = x.shape
    m = torch.full((B, T, HW), float("nan"), device="cuda")
    fr, af = torch.full((B, T), float("nan"), device="cuda"), torch.full((B, T), float("nan"), device="cuda")
    tot = torch.full((B,), float("nan"), device="cuda")
    xd, bd, gd = _dev(x), _dev(base), _dev(gsum)
    L.check(lib.ivf_ig_finish(L.ptr(xd), kind, L.ptr(bd), value, L.ptr(gd), B, C, T, HW, L.ptr(m), L.ptr(fr), L.ptr(af),
                              L.ptr(tot), L.stream()))
    return {"map": m.cpu().numpy(), "frames": fr.cpu().numpy(), "abs_frames": af.cpu().numpy(), "total": tot.cpu().numpy()}


@pytest.mark.parametrize("kind", list(R.KINDS.values()), ids=list(R.KINDS))
def test_finish_matches_fp64(kind):
    L, lib = _lib()
    for shape in R.ACC_SHAPES:
        B, C, T, HW, K = shape
        x, base, value, gsum = R.finish_inputs(shape, kind)
        x0 = R.baseline(x, kind, base, value)
        f = R.finish_ref(x, x0, gsum)
        got = _finish(L, lib, x, kind, base, value, gsum)
        figs = []
        for name, bname in (("map", "b_map"), ("frames", "b_frames"), ("abs_frames", "b_frames"), ("total", "b_total")):
            err = np.abs(got[name].astype(F64) - f[name])
            figs.append(f"{name} {float(np.max(err / np.maximum(f[bname], 1e-300))):.3f}")
            assert not np.isnan(got[name]).any() and np.all(err <= f[bname]), (shape, name)
        note(f"ig finish {shape} kind {kind}: share of the bound used: " + ", ".join(figs))
        if kind == R.FROZEN:
            assert not got["map"][:, 0].any() and not got["frames"][:, 0].any() and not got["abs_frames"][:, 0].any()
        for r in range(B):
            solo = _finish(L, lib, x[r:r + 1], kind, None if base is None else base[r:r + 1], value, gsum[r:r + 1])
            for name in got:
                assert _same_bits(solo[name][0], got[name][r]), (shape, r, name)


# ---------------------------------------------------------------------------------------------------- the ConvLSTM chain
def _clstm_engine(case, max_batch, sd):
    import ivf_engine
    eng = ivf_engine.CLSTMEngine(CR.K, (case.C, case.T, case.H, case.W), max_batch=max_batch, hidden=case.hid,
                                 layers=case.layers, kernel=case.k, stride=case.s, softmax=case.softmax,
                                 batch_norm=case.batch_norm)
    eng.load_state_dict(sd)
    return eng


def _host(res):
    return {k: v.detach().cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("name", [b[0] for b in R.CHAIN_BASELINES])
def test_chain_matches_fp64_autograd(name):
    """Case S2, K = 4: ig_map, frames, total and the path scores of every clip against torch fp64 autograd through
    clstm_refs' functional model, at GATE_MARGIN x the float32 floor of the same tensor.  ig_total is held to the
    reference's ig_total: the quadrature gap to f(x) - f(x0) belongs to the reference and is only recorded."""
    b = R.chain_reference(name)
    assert int(b["ambiguous"].sum()) == 0                     # no clip is left out (test_ig_refs_host.py)
    case, x = b["case"], torch.from_numpy(b["x"]).cuda()
    eng = _clstm_engine(case, case.B, b["sd"])
    got = _host(eng.ig(x, b["targets"], steps=R.CHAIN_K, baseline=name))
    ref = b["ref"]
    pairs = {"map": got["ig_map"].reshape(ref["map"].shape), "frames": got["ig_frames"], "total": got["ig_total"],
             "path_scores": got["path_scores"]}
    worst = {n: float(np.max(R.chain_err(v, ref[n]))) for n, v in pairs.items()}
    for n, v in worst.items():
        note(f"ig chain {name} {n}: floor {b['floor'][n]:.3e} gpu {v:.3e} ratio {v / b['floor'][n]:.2f} "
             f"(gate {CR.GATE_MARGIN:g}x)")
    note(f"ig chain {name}: ig_total gpu {got['ig_total'].tolist()} ref {ref['total'].tolist()}, gpu f(x) - f(x0) "
         f"{(got['score_x'] - got['score_base']).tolist()}, gpu ig_gap {got['ig_gap'].tolist()}")
    for n, v in worst.items():
        assert v <= b["gate"][n], (name, n, v, b["gate"][n])
    if name == "frozen":
        assert not got["ig_map"][:, 0].any() and not got["ig_frames"][:, 0].any()
    assert np.array_equal(got["ig_gap"], got["ig_total"] - (got["score_x"] - got["score_base"]))


# ---------------------------------------------------------------------------------------------------- driver == pieces
def test_driver_equals_its_pieces_and_one_clip_calls():
    """ivf_clstm_ig on a plan of 3 rows, b = 2, K = 4 (chunks of 3 rows cross the clip boundary) equals the kernels
    called one by one around the plan's forward and backward, and equals one-clip calls, bit for bit"""
    L, lib = _lib()
    case, x, sd, targets = R.chain_inputs()
    eng = _clstm_engine(case, 3, sd)
    K, b = R.CHAIN_K, x.shape[0]
    C, T, H, W = eng.clip_shape
    HW = H * W
    alpha, w = R.midpoint(K)
    xd, ad, wd = _dev(x), _dev(alpha), _dev(w)
    for name, kind, value in R.CHAIN_BASELINES:
        whole = _host(eng.ig(xd, targets, steps=K, baseline=name, base=value if name == "constant" else None))
        G = torch.zeros(b, C, T, HW, device="cuda")
        scores = torch.empty(b * K, device="cuda")
        rowt = [t for t in targets for _ in range(K)]
        for first in range(0, b * K, eng.max_batch):
            cnt = min(eng.max_batch, b * K - first)
            p = torch.empty(cnt, C, T, H, W, device="cuda")
            L.check(lib.ivf_ig_stage(L.ptr(xd), kind, None, value, L.ptr(ad), b, C, T, HW, K, first, cnt, L.ptr(p), 0, L.stream()))
            eng.forward(p)
            sc, dx = eng.backward(cnt, target=rowt[first:first + cnt])
            scores[first:first + cnt] = sc
            L.check(lib.ivf_ig_accumulate(L.ptr(dx), 0, L.ptr(wd), K, first, cnt, L.ptr(G), b, C, T, HW, L.stream()))
        parts = _finish(L, lib, x.reshape(b, C, T, HW), kind, None, value, G.cpu().numpy())
        assert _same_bits(whole["ig_map"].reshape(b, T, HW), parts["map"])
        assert _same_bits(whole["ig_frames"], parts["frames"]) and _same_bits(whole["ig_abs_frames"], parts["abs_frames"])
        assert _same_bits(whole["ig_total"], parts["total"])
        assert _same_bits(whole["path_scores"], scores.cpu().numpy().reshape(b, K))
        ps = eng.ig_path_scores(xd, targets, baseline=name, alpha=alpha).cpu().numpy()
        assert _same_bits(ps, whole["path_scores"])
        for r in range(b):
            solo = _host(eng.ig(xd[r:r + 1], targets[r:r + 1], steps=K, baseline=name))
            for key in whole:
                assert _same_bits(solo[key][0], whole[key][r]), (name, r, key)
    # an explicit baseline clip equal to the frozen clip is the frozen baseline
    frozen = _host(eng.ig(xd, targets, steps=K, baseline="frozen"))
    clip = _host(eng.ig(xd, targets, steps=K, baseline="clip", base=xd[:, :, :1].expand_as(xd).contiguous()))
    for key in frozen:
        assert _same_bits(frozen[key], clip[key]), key
    with pytest.raises(L.IvfError):
        eng.ig(xd, targets, baseline="clip")
    with pytest.raises(L.IvfError):
        eng.ig(xd, targets, baseline="grey")
    with pytest.raises(L.IvfError):
        eng.ig(xd, targets, alpha=[0.5])                       # nodes without weights


# ---------------------------------------------------------------------------------------------------- I3D against the fixture
@pytest.mark.parametrize("math", ["fp32", "bf16x3", "bf16x6"])
def test_i3d_matches_fixture(math, golden):
    """Clips 21 and 7 in one call on a plan of 3 rows, K = 8: the sampled map and abs_frames at the whole-chain
    d(score)/d(input) gates of test_gpu_i3d.py; frames, total and ig_gap -- cancellation figures, sum|A| is 40-110
    against totals of 0.007-0.48 -- at that gate times the fixture's abs_frames.

    Measured on the MI355X (DESIGN 13 has the table), worst over clips and baselines: map L2 / max 7.7e-3 / 1.4e-2
    (fp32), 6.3e-3 / 1.2e-2 (bf16x6), 1.9e-2 / 2.5e-2 (bf16x3); frames within 1.1e-4 of abs_frames, total and ig_gap
    within 1.4e-5 of their sum.  The figures are written by note() on every run."""
    import ivf_engine
    import ivf_recipe as RC
    g = golden("ig")
    K = int(g["K"])
    exact = math in R.I3D_EXACT
    l2_gate, max_gate = R.I3D_L2_GATE[exact], R.I3D_MAX_GATE[exact]
    eng = ivf_engine.I3DEngine(174, (3, 16, 224, 224), max_batch=3, softmax=True, math=math)
    eng.load_state_dict(RC.i3d_state_dict(num_classes=174))
    x = torch.from_numpy(np.stack([RC.clip(c) for c in R.I3D_CLIPS])).cuda()
    targets = [int(g[f"c{c}_target"]) for c in R.I3D_CLIPS]
    fails = []
    for tag, baseline, base in R.I3D_BASELINES:
        got = _host(eng.ig(x, targets, steps=K, baseline=baseline, base=base))
        for i, cid in enumerate(R.I3D_CLIPS):
            p = f"c{cid}_{tag}"
            ref, af = g[f"{p}_map_val"].astype(F64), g[f"{p}_abs_frames"]
            sample = got["ig_map"][i].ravel()[g[f"{p}_map_idx"]].astype(F64)
            l2 = np.linalg.norm(sample - ref) / np.linalg.norm(ref)
            mx = rel_err(sample, ref)
            pos = af > 0
            ea = float(np.max(np.abs(got["ig_abs_frames"][i] - af)[pos] / af[pos]))
            ef = float(np.max(np.abs(got["ig_frames"][i] - g[f"{p}_frames"])[pos] / af[pos]))
            et = abs(float(got["ig_total"][i]) - float(g[f"{p}_total"])) / af.sum()
            gap_ref = float(g[f"{p}_total"]) - (float(g[f"{p}_score_x"]) - float(g[f"{p}_score_base"]))
            eg = abs(float(got["ig_gap"][i]) - gap_ref) / af.sum()
            es = rel_err(got["path_scores"][i], g[f"{p}_path_scores"])
            note(f"ig i3d {math} {p}: map L2 {l2:.2e} max {mx:.2e} (gates {l2_gate:g} {max_gate:g}); abs_frames {ea:.2e}, "
                 f"frames/abs_frames {ef:.2e}, total/sum abs_frames {et:.2e}, gap/sum abs_frames {eg:.2e} (gate {l2_gate:g}); "
                 f"path scores {es:.2e}; total {float(got['ig_total'][i]):.6f} ref {float(g[f'{p}_total']):.6f}, "
                 f"gap {float(got['ig_gap'][i]):.3e} ref {gap_ref:.3e}")
            checks = {"map L2": l2 < l2_gate, "map max": mx < max_gate, "abs_frames": ea < l2_gate, "frames": ef < l2_gate,
                      "total": et < l2_gate, "gap": eg < l2_gate, "path scores": es < 1e-3,
                      "score_x": abs(float(got["score_x"][i]) - float(g[f"{p}_score_x"])) < 1e-3 * float(g[f"{p}_score_x"]),
                      "score_base": abs(float(got["score_base"][i]) - float(g[f"{p}_score_base"]))
                      < 1e-3 * max(float(g[f"{p}_score_base"]), float(g[f"{p}_score_x"]))}
            fails += [(p, n) for n, ok in checks.items() if not ok]
            if tag == "frozen":
                assert not got["ig_map"][i, 0].any() and got["ig_frames"][i, 0] == 0 and got["ig_abs_frames"][i, 0] == 0
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------- surfaces
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


def test_integrated_gradients_video_i3d(smth_model):
    import ivf_recipe as RC
    from integrated_gradients_videos import IntegratedGradientsVideo
    x = torch.from_numpy(RC.clip(21))[None]
    igv = IntegratedGradientsVideo(smth_model, steps=4)
    m, out = igv(x)
    assert m.shape == (16, 224, 224) and m.dtype == np.float32 and tuple(out.shape) == (1, 174)
    assert not m[0].any() and np.isfinite(m).all() and m[1:].any()
    eng = smth_model._engine_for(x.cuda())
    pred = int(torch.argmax(out[0]))
    want = eng.ig(x.cuda(), [pred], steps=4)["ig_map"][0].cpu().numpy()
    assert _same_bits(m, want)                                   # index None = the argmax
    m3, _ = IntegratedGradientsVideo(smth_model, steps=4, baseline="constant")(x, index=3)
    assert m3[0].any() and not _same_bits(m3, m)
    assert abs(float(igv.last["ig_total"][0]) - float(m.astype(F64).sum())) <= sum_bound(float(np.abs(m).sum()), m.size)


def test_integrated_gradients_video_clstm():
    import ivf_recipe as RC
    from integrated_gradients_videos import IntegratedGradientsVideo
    model = _kth_clstm()
    x = torch.from_numpy(RC.clip(7, 3, 32, 120, 160))[None]
    igv = IntegratedGradientsVideo(model, steps=4, archType="CLSTM")
    m, out = igv(x, index=2)
    assert m.shape == (32, 120, 160) and m.dtype == np.float32 and tuple(out.shape) == (1, 6)
    assert not m[0].any() and np.isfinite(m).all() and m[1:].any()
    for k in ("ig_frames", "ig_abs_frames", "path_scores", "score_x", "score_base", "ig_gap"):
        assert k in igv.last
    import ivf_lib as L
    with pytest.raises(L.IvfError):
        IntegratedGradientsVideo(model, archType="VGG")(x)


def _check_ig_records(ig, tm, T, H, W, n):
    assert len(ig) == len(tm) == n
    for rec, trec in zip(ig, tm):
        assert set(rec) == {'true_class', 'pred_class', 'video_id', 'IGHeatMap', 'IGFrames', 'ig_total', 'ig_gap',
                            'score_base'}
        assert rec['IGHeatMap'].shape == (T, H, W) and rec['IGHeatMap'].dtype == np.float32
        assert rec['IGFrames'].shape == (T,) and rec['pred_class'] == trec['pred_class']
        m = rec['IGHeatMap'].astype(F64)
        bound = sum_bound(np.abs(m).sum((1, 2)), H * W) + U * np.abs(rec['IGFrames'])
        assert np.all(np.abs(rec['IGFrames'] - m.sum((1, 2))) <= bound)
        assert not rec['IGHeatMap'][0].any()                     # 'frozen': frame 0 attributes exactly 0
        assert abs(rec['ig_total'] - float(rec['IGFrames'].astype(F64).sum())) <= sum_bound(np.abs(rec['IGFrames']).sum(), T)
        assert all(isinstance(rec[k], float) for k in ('ig_total', 'ig_gap', 'score_base'))


def test_smth_driver_with_intgrad(smth_model, tmp_path, monkeypatch):
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(drv._state, "sub_dir", "run0")     # a driver's main() run earlier in the process leaves its own
    loader = ivf_find_masks.SyntheticLoader(2, 2, (3, 16, 224, 224), 174, first_id=40)
    hp = {"batch_size": 2, "gradCamType": "guessed"}
    drv.find_masks(loader, smth_model, hp, 0.01, 0.02, 2, "central", "freeze", classOI=None, doGradCam=False,
                   runTempMask=True, verbose=False, doIntGrad=True, igSteps=4)
    tm = pickle.load(open(tmp_path / "results" / "allTimeMaskResults_run0_None_.p", "rb"))
    ig = pickle.load(open(tmp_path / "results" / "allIntGradResults_run0_None_.p", "rb"))
    _check_ig_records(ig, tm, 16, 224, 224, 2)
    assert pickle.load(open(tmp_path / "results" / "allGradCamResults_run0_None_.p", "rb")) == []
    assert ig[0]['video_id'] == 40
    strips = [p for p in (tmp_path / "cam_saved_images").rglob("intgrad/*.png")]
    assert any(p.name == "casefreeze40_15.png" for p in strips) and any(p.name == "casereverse41_0.png" for p in strips)
    from PIL import Image
    f0 = np.asarray(Image.open(next(p for p in strips if p.name == "casefreeze40_0.png")))
    assert f0.shape == (224, 3 * 224, 3)                         # frame 0's heat map is all zero, and blends finite
    # all zero blends as the colour map's entry 0 over the frame, never NaN: the middle panel is not black
    assert f0[:, 224:448].any()
    assert len(list((tmp_path / "cam_saved_images").rglob("intgrad/mygif.gif"))) == 2


def test_kth_driver_with_intgrad_on_the_convlstm(tmp_path, monkeypatch):
    import FindMasksComparison_I3D_KTH as drv
    import ivf_find_masks
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(drv._state, "sub_dir", "run0")     # a driver's main() run earlier in the process leaves its own
    loader = ivf_find_masks.SyntheticLoader(1, 1, (3, 32, 120, 160), 6, first_id=7)
    drv.find_masks(loader, _kth_clstm(), {"batch_size": 1, "gradCamType": "guessed"}, 0.02, 0.04, 2, 1, "central",
                   "freeze", classOI=None, doGradCam=False, runTempMask=True, verbose=False, doIntGrad=True, igSteps=4,
                   igBaseline="frozen")
    tm = pickle.load(open(tmp_path / "results" / "I3d_KTH_allTimeMaskResults_original_run0.p", "rb"))
    ig = pickle.load(open(tmp_path / "results" / "I3d_KTH_allIntGradResults_original_run0.p", "rb"))
    _check_ig_records(ig, tm, 32, 120, 160, 1)
    assert ig[0]['video_id'] == "7"
    assert len(list((tmp_path / "cam_saved_images").rglob("intgrad/mygif.gif"))) == 1


def test_records_are_byte_identical_with_intgrad_off(smth_model, tmp_path, monkeypatch):
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    blobs = []
    for sub, extra in (("plain", {}), ("kwargs", dict(doIntGrad=False, igSteps=7, igBaseline="constant"))):
        d = tmp_path / sub
        d.mkdir()
        monkeypatch.chdir(d)
        loader = ivf_find_masks.SyntheticLoader(1, 1, (3, 16, 224, 224), 174, first_id=40)
        drv.find_masks(loader, smth_model, {"batch_size": 1, "gradCamType": "guessed"}, 0.01, 0.02, 2, "central",
                       "freeze", classOI=None, doGradCam=True, runTempMask=True, verbose=False, **extra)
        files = sorted(p.relative_to(d) for p in d.rglob("*") if p.is_file())
        blobs.append({str(p): (d / p).read_bytes() for p in files})
        assert not any("IntGrad" in str(p) or "intgrad" in str(p) for p in files)
    assert blobs[0].keys() == blobs[1].keys()
    assert all(blobs[0][k] == blobs[1][k] for k in blobs[0]), [k for k in blobs[0] if blobs[0][k] != blobs[1][k]]


def test_tf_plan_refuses():
    import ivf_engine
    import ivf_lib as L
    eng = ivf_engine.TFCLSTMEngine(6, (1, 4, 30, 40), units=(4,), kernel=(3, 5), stride=2, padding="valid", max_batch=1)
    x = torch.zeros(1, 1, 4, 30, 40, device="cuda")
    with pytest.raises(L.IvfError):
        eng.ig(x, [0])
    with pytest.raises(L.IvfError):
        eng.ig_path_scores(x, [0])
