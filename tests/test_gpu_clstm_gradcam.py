"""GPU: Grad-CAM of the ConvLSTM backbone (archType='CLSTM', csrc/convlstm.hip) against tests/golden/clstm_gradcam.npz
(the reference's CLSTM_4.Model + torch autograd + the reference's own Grad-CAM arithmetic, see
tests/golden/make_golden_clstm_gradcam.py).

Target 'clstm' (layer=None) is the reference's branch: top layer at the effective steps.  Targets 'cell<i>'
(layer=i) are the per-frame extension.  Gates: 1e-3 absolute on the normalised maps (the project's Grad-CAM gate),
1e-3 relative to max|.| (conftest.rel_err) on probabilities, channel weights and raw maps.
"""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import note, rel_err

pytestmark = pytest.mark.gpu

T, EFF = 32, [7, 15, 23, 31]
GATE = 1e-3


def _sd(entire):
    import ivf_recipe as R
    return R.clstm_state_dict(channels=3, tag='clstm3', fc_mult=4 if entire else 1)


def _engine(entire=False, softmax=False, B=1, hidden=4, sd=None):
    import ivf_engine
    eng = ivf_engine.CLSTMEngine(6, (3, T, 120, 160), max_batch=B, hidden=hidden, layers=2, kernel=5, stride=2,
                                 softmax=softmax, out_step=EFF[-1], out_steps=EFF if entire else None,
                                 effective_steps=EFF)
    eng.load_state_dict(sd if sd is not None else _sd(entire))
    return eng


def _clip(cid=7):
    import ivf_recipe as R
    return torch.from_numpy(R.clip(cid, 3, T, 120, 160) / 255.0).float()[None].cuda()


def _model(entire=False, softmax=False):
    import ivf_recipe as R
    from models import CLSTM_4
    m = CLSTM_4.Model(num_classes=6, nb_lstm_units=4, channels=3, conv_kernel_size=(5, 5), lstm_layers=2, step=T,
                      image_size=(160, 120), conv_stride=2, effective_step=EFF, use_entire_seq=entire,
                      add_softmax=softmax)
    m.load_state_dict(R.to_torch(_sd(entire)))
    return m.cuda().eval()


LAYERS = {"clstm": None, "cell0": 0, "cell1": 1}


@pytest.mark.parametrize("name", ["clstm", "cell0", "cell1"])
@pytest.mark.parametrize("softmax", [0, 1])
@pytest.mark.parametrize("entire", [0, 1])
def test_gradcam_matches_reference(entire, softmax, name, golden):
    """(1) probabilities, channel weights, raw maps and the final maps for both normalisations."""
    g = golden("clstm_gradcam")
    key = f"e{entire}_s{softmax}_{name}"
    eng = _engine(bool(entire), bool(softmax))
    x = _clip()
    layer = LAYERS[name]
    raw = eng.gradcam_raw(x, None, layer=layer)                  # target None: argmax on the device
    probs = raw["probs"].cpu().numpy()
    assert int(probs.argmax()) == int(g[key + "_index"])
    w = raw["weights"][0].cpu().numpy()
    cam = raw["cam"][0].cpu().numpy()
    n = len(EFF) if layer is None else T
    assert cam.shape[0] == n and raw["feat"].shape == raw["grad"].shape == (1, n, 4) + cam.shape[1:]
    if name == "cell0":
        cam = cam[::2, ::2, ::2]
    errs = dict(probs=rel_err(probs, g[key + "_probs"]), w=rel_err(w, g[key + "_w"]), cam=rel_err(cam, g[key + "_cam"]))
    for pf in (1, 0):
        got, pr = eng.gradcam(x, [int(g[key + "_index"])], per_frame=bool(pf), out_hw=(120, 160), layer=layer)
        assert got.shape == (1, T, 120, 160)
        got = got[0].cpu().numpy()
        assert np.isfinite(got).all()
        got = got[:, ::8, ::8] if pf else got[::4, ::8, ::8]
        errs[f"map_pf{pf}"] = float(np.max(np.abs(got - g[f"{key}_pf{pf}"])))
        assert np.array_equal(pr.cpu().numpy(), probs)
    note(f"clstm_gradcam {key}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < GATE, f"{key}: {k} off by {v:.3e}"


@pytest.mark.parametrize("hid,plane", [(1, 7), (4, 35), (4, 1200), (32, 70), (32, 299)])
def test_reduce_kernel_matches_numpy(hid, plane):
    """(2) ivf_clstm_gradcam_reduce on random arrays against float64 numpy: step lists with gaps, odd planes."""
    import ivf_lib as L
    B, Tn = 3, 9
    rng = np.random.default_rng(hid * 1000 + plane)
    feat = rng.standard_normal((B, Tn, hid, plane)).astype(np.float32)
    grad = (rng.standard_normal((B, Tn, hid, plane)) * 1e-3).astype(np.float32)
    for steps in (None, [0, 3, 4, 8], [5]):
        sel = list(range(Tn)) if steps is None else steps
        n = len(sel)
        f, gr = torch.from_numpy(feat).cuda(), torch.from_numpy(grad).cuda()
        w = torch.full((B, hid), float("nan"), device="cuda")
        cam = torch.full((B, n, plane), float("nan"), device="cuda")
        arr = (ctypes.c_int * n)(*sel) if steps is not None else None
        L.check(L.lib().ivf_clstm_gradcam_reduce(L.ptr(f), L.ptr(gr), arr, n, L.ptr(w), L.ptr(cam), B, Tn, hid, plane,
                                                 L.stream()))
        torch.cuda.synchronize()
        w_ref = grad.astype(np.float64)[:, sel].mean(axis=(1, 3))
        # the maps are compared with the kernel's own fp32 weights, so that the gate measures the weighted sum
        w_got = w.cpu().numpy()
        cam_ref = np.maximum(np.einsum("bc,bncp->bnp", w_got.astype(np.float64), feat.astype(np.float64)[:, sel]), 0)
        # fp32 weights of a mean of n*plane terms of size ~1e-3: absolute error far below 1e-9
        assert np.max(np.abs(w_got - w_ref)) < 1e-6 * np.max(np.abs(grad)), (hid, plane, steps)
        assert rel_err(cam.cpu().numpy(), cam_ref) < 1e-5, (hid, plane, steps)
    bad = (ctypes.c_int * 1)(Tn)
    assert L.lib().ivf_clstm_gradcam_reduce(L.ptr(f), L.ptr(gr), bad, 1, L.ptr(w), L.ptr(cam), B, Tn, hid, plane,
                                            L.stream()) == -1


def _check_truncation(eng, x, tgt, steps):
    """gradcam_raw(layer=i) must read exactly what a full backward leaves for layer i."""
    b = x.shape[0]
    for layer in range(eng.layers):
        eng.forward(x)
        eng.backward(b, target=tgt)
        X, dX = eng.layer_state(layer, b)
        raw = eng.gradcam_raw(x, tgt, layer=layer)
        assert torch.equal(raw["grad"], dX) and torch.equal(raw["feat"], X), layer
        assert float(dX.abs().max()) > 0
    raw = eng.gradcam_raw(x, tgt, layer=None)            # X, dX: the top layer's, from the last round
    assert torch.equal(raw["grad"], dX[:, steps]) and torch.equal(raw["feat"], X[:, steps])


@pytest.mark.parametrize("persist", ["0", "1"])
def test_truncated_backward_equals_full_backward(persist):
    """(3) the gradients gradcam_raw reads equal, bit for bit, what a full backward leaves for that layer.
    The recurrence path (step kernels / persistent) is read from IVF_CLSTM_PERSIST once per process, so each
    path runs in one child process."""
    import subprocess
    import sys
    code = (
        "import sys, torch\n"
        f"sys.path[:0] = {[os.path.dirname(os.path.abspath(__file__))]!r}\n"
        "import conftest, test_gpu_clstm_gradcam as t\n"
        "eng = t._engine(True, True, B=2)\n"
        "t._check_truncation(eng, torch.cat([t._clip(7), t._clip(8)]), [2, 1], t.EFF)\n"
        "print('ok')\n")
    env = dict(os.environ, IVF_CLSTM_PERSIST=persist)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_truncated_backward_wide_path():
    """(3) on the wide kernels (hidden > 4), one input channel, a small geometry."""
    import ivf_engine
    import ivf_recipe as R
    sd = R.clstm_state_dict(num_classes=5, hidden=8, channels=1, kernel=5, layers=2, image_size=(64, 128),
                            conv_stride=2, tag="clstm_cam_wide")
    eng = ivf_engine.CLSTMEngine(5, (1, 8, 128, 64), max_batch=2, hidden=8, layers=2, kernel=5, stride=2,
                                 softmax=True, out_step=7, effective_steps=[3, 7])
    eng.load_state_dict(sd)
    x = torch.from_numpy(np.stack([R.clip(c, 1, 8, 128, 64) / 255.0 for c in (1, 2)])).float().cuda()
    _check_truncation(eng, x, [0, 4], [3, 7])
    cam, probs = eng.gradcam(x, None, per_frame=False, layer=None)
    assert tuple(cam.shape) == (2, 8, 128, 64) and tuple(probs.shape) == (2, 5)


def _same_bits(a, b):
    """Bit-for-bit equality, NaN included (a frame whose raw map is all zero normalises to 0/0, as in the
    reference; clips 8 and 9 with the arbitrary classes below have such frames)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_batch_independence(golden):
    """(4) row j of a 3-clip call equals the 1-clip call bit for bit (same recurrence path); a b = 64 call
    (persistent recurrence) agrees with b = 1 within the gate (clip 7 with its predicted class, the fixture's
    case, whose maps all have a positive maximum)."""
    eng = _engine(False, True, B=64)
    clips = torch.cat([_clip(7), _clip(8), _clip(9)])
    tgt = [0, 3, 5]
    for layer in (None, 0, 1):
        three = eng.gradcam_raw(clips, tgt, layer=layer)
        cam3, _ = eng.gradcam(clips, tgt, per_frame=True, out_hw=(120, 160), layer=layer)
        for j in range(3):
            one = eng.gradcam_raw(clips[j:j + 1], tgt[j:j + 1], layer=layer)
            for k in ("cam", "weights", "feat", "grad", "probs"):
                assert _same_bits(one[k][0], three[k][j]), (layer, j, k)
            cam1, _ = eng.gradcam(clips[j:j + 1], tgt[j:j + 1], per_frame=True, out_hw=(120, 160), layer=layer)
            assert _same_bits(cam1[0], cam3[j]), (layer, j)
        big = clips[:1].expand(64, -1, -1, -1, -1).contiguous()
        many = eng.gradcam_raw(big, [tgt[0]] * 64, layer=layer)
        one = eng.gradcam_raw(clips[:1], tgt[:1], layer=layer)
        cam64, _ = eng.gradcam(big, [tgt[0]] * 64, per_frame=True, out_hw=(120, 160), layer=layer)
        cam1, _ = eng.gradcam(clips[:1], tgt[:1], per_frame=True, out_hw=(120, 160), layer=layer)
        ew = rel_err(many["weights"][63].cpu().numpy(), one["weights"][0].cpu().numpy())
        ec = rel_err(many["cam"][63].cpu().numpy(), one["cam"][0].cpu().numpy())
        em = float((cam64[63] - cam1[0]).abs().max())
        note(f"clstm_gradcam b=64 vs b=1 layer {layer}: w {ew:.2e} cam {ec:.2e} map {em:.2e}")
        assert _same_bits(many["cam"][0], many["cam"][63])           # rows of one call do not differ either
        assert ew < GATE and ec < GATE and em < GATE


def test_gradcam_video_dropin(golden):
    """(5) GradCamVideo / FeatureExtractor with archType='CLSTM'."""
    import grad_cam_videos as gcv
    import ivf_lib as L
    g = golden("clstm_gradcam")
    m = _model(False, False)
    x = _clip()
    for name, n, hw in (("clstm", 4, (7, 10)), ("cell0", T, (30, 40))):
        gc = gcv.GradCamVideo(model=m, target_layer_names=[name], class_dict=None, use_cuda=True,
                              input_spatial_size=(160, 120), normalizePerFrame=True, archType="CLSTM")
        cam, out = gc(x, None)
        assert cam.shape == (T, 120, 160) and cam.dtype == np.float32 and tuple(out.shape) == (1, 6)
        err = float(np.max(np.abs(cam[:, ::8, ::8] - g[f"e0_s0_{name}_pf1"])))
        note(f"clstm_gradcam GradCamVideo {name}: map {err:.2e}")
        assert err < GATE
        assert rel_err(out.cpu().numpy(), g[f"e0_s0_{name}_probs"]) < GATE
        fe = gcv.FeatureExtractor(m, [name], "CLSTM")
        acts, y = fe(x)
        assert len(acts) == 1 and tuple(acts[0].shape) == (n, 1, 4) + hw and tuple(y.shape) == (1, 6)
        assert len(fe.gradients) == 1 and fe.gradients[0].shape == acts[0].shape
        acts2, y2 = gcv.ModelOutputsVideo(m, [name], "CLSTM")(x)
        assert torch.equal(acts2[0], acts[0]) and torch.equal(y2, y)
    for bad in (["clstm", "cell0"], ["cell7"], ["Mixed_5c"]):
        with pytest.raises(L.IvfError):
            gcv.GradCamVideo(model=m, target_layer_names=bad, class_dict=None, use_cuda=True,
                             input_spatial_size=(160, 120), archType="CLSTM")(x, None)
        with pytest.raises(L.IvfError):
            gcv.FeatureExtractor(m, bad, "CLSTM")(x)
    with pytest.raises(L.IvfError):
        gcv.GradCamVideo(model=m, target_layer_names=["clstm"], class_dict=None, use_cuda=True,
                         input_spatial_size=(160, 120), archType="VGG")(x, None)


def test_mask_search_with_gradcam():
    """(6a) MaskSearch on a CLSTMEngine with do_gradcam=True (its default)."""
    import ivf_search
    eng = _engine(False, True, B=2)
    x = torch.cat([_clip(7), _clip(8)])
    res = ivf_search.MaskSearch(eng, 0.02, 0.04, 3, "freeze", gradcam_size=(120, 160)).run(x, [1, 2])
    cam = res["gradcam"]
    assert tuple(cam.shape) == (2, T, 120, 160)
    assert bool(torch.isfinite(cam).all()) and float(cam.min()) >= 0 and float(cam.max()) <= 1
    want, _ = eng.gradcam(x, res["pred_class"], per_frame=True, out_hw=(120, 160))
    assert torch.equal(cam, want)


def test_kth_driver_writes_gradcam_for_the_convlstm(tmp_path, monkeypatch):
    """(6b) FindMasksComparison_I3D_KTH.find_masks(doGradCam=True) with a CLSTM_4 model: GCHeatMap records, both
    pickles, the heat-map strips of both perturbation types."""
    import FindMasksComparison_I3D_KTH as drv
    import ivf_find_masks
    monkeypatch.chdir(tmp_path)
    m = _model(False, False)
    loader = ivf_find_masks.SyntheticLoader(2, 2, (3, T, 120, 160), 6, first_id=7)
    cfg = {"batch_size": 2, "gradCamType": "guessed"}
    masks = drv.find_masks(loader, m, cfg, 0.02, 0.04, 4, 1, "central", "freeze", classOI=None, doGradCam=True,
                           runTempMask=True, verbose=False)
    assert len(masks) == 2
    tm = pickle.load(open(tmp_path / "results" / "I3d_KTH_allTimeMaskResults_original_run0.p", "rb"))
    gc = pickle.load(open(tmp_path / "results" / "I3d_KTH_allGradCamResults_original_run0.p", "rb"))
    assert len(tm) == 2 and len(gc) == 2
    for rec in gc:
        hm = rec["GCHeatMap"]
        assert hm.shape == (T, 120, 160) and hm.dtype == np.float32
        assert np.isfinite(hm).all() and hm.min() >= 0 and hm.max() <= 1
    assert [r["video_id"] for r in gc] == ["7", "8"]
    names = {p.name for p in (tmp_path / "cam_saved_images").rglob("*") if p.is_file()}
    for kind in ("freeze", "reverse"):
        for vid in ("7", "8"):
            assert f"MASKVALScase{kind}{vid}.txt" in names
            assert any(f.startswith(f"case{kind}{vid}_") and f.endswith(".png") for f in names), kind
    assert "img32.jpg" in names and "mygif.gif" in names
