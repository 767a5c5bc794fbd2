"""CPU: Grad-CAM of the ConvLSTM (archType='CLSTM') -- the C-ABI carries the new entry points, the fixture
tests/golden/clstm_gradcam.npz is consistent with itself, and the argument checks that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("ivf_clstm_gradcam_reduce", "ivf_clstm_set_cam_steps", "ivf_clstm_gradcam", "ivf_clstm_gradcam_raw",
       "ivf_clstm_layer_buffers")
T, EFF = 32, [7, 15, 23, 31]


def test_new_symbols_in_header_library_and_binding():
    import ivf_lib
    text = open(os.path.join(ROOT, "include", "ivf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(ivf_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} not declared in include/ivf_hip.h"
        assert hasattr(lib, n), f"{n} not exported"
        assert n in ivf_lib.exported_symbols()
        assert getattr(ivf_lib.lib(), n).argtypes is not None


def _plan(B=2, hidden=4, layers=2):
    import ivf_lib as L
    cfg = L.CLSTMConfig()
    cfg.B, cfg.C, cfg.T, cfg.H, cfg.W = B, 3, T, 120, 160
    cfg.hidden, cfg.layers, cfg.kernel, cfg.stride, cfg.num_classes = hidden, layers, 5, 2, 6
    cfg.batch_norm, cfg.out_step = 1, T - 1
    h = ctypes.c_void_p()
    L.check(L.lib().ivf_clstm_create(ctypes.byref(cfg), ctypes.byref(h)))
    return h


def test_argument_checks_without_a_device():
    import ivf_lib as L
    lib = L.lib()
    assert lib.ivf_clstm_gradcam_reduce(None, None, None, 4, None, None, 1, T, 4, 70, None) == -1
    assert b"clstm_gradcam_reduce" in lib.ivf_last_error()
    h = _plan()
    ok = (ctypes.c_int * 4)(*EFF)
    assert lib.ivf_clstm_set_cam_steps(h, ok, 4) == 0
    for bad in ([7, 7], [15, 7], [7, T], [-1, 3]):
        assert lib.ivf_clstm_set_cam_steps(h, (ctypes.c_int * len(bad))(*bad), len(bad)) == -1, bad
    assert lib.ivf_clstm_set_cam_steps(h, ok, 0) == -1 and lib.ivf_clstm_set_cam_steps(h, None, 4) == -1
    # an unbound plan computes nothing: every entry refuses before it launches
    assert lib.ivf_clstm_gradcam(h, None, 1, None, -1, 1, 120, 160, None, None, None) == -1
    assert lib.ivf_clstm_gradcam_raw(h, None, 1, None, 0, None, None, None, None, None, None) == -1
    assert lib.ivf_clstm_layer_buffers(h, 0, None, None, None, None, None) == -1       # not bound
    lib.ivf_clstm_destroy(h)


def test_workspace_reserves_the_gradcam_scratch():
    """cam [B,T,Hp0,Wp0] + weights [B,hid] + min/max [B,T,2] + targets [B] sit in the plan's workspace and scale
    with B."""
    import ivf_lib as L
    lib = L.lib()
    h1, h2 = _plan(B=1), _plan(B=3)
    w1, w2 = lib.ivf_clstm_workspace_bytes(h1), lib.ivf_clstm_workspace_bytes(h2)
    cam = T * 30 * 40 * 4
    assert w2 - w1 >= 2 * cam and w1 > cam
    lib.ivf_clstm_destroy(h1)
    lib.ivf_clstm_destroy(h2)


def test_target_names_are_parsed_without_a_device():
    import grad_cam_videos as gcv
    import ivf_lib as L

    class M:
        lstm_layers = 2
    assert gcv._clstm_layer(M, "clstm") is None and gcv._clstm_layer(M, "cell0") == 0 and gcv._clstm_layer(M, "cell1") == 1
    for bad in ("cell2", "cell7", "Mixed_5c", "cell", "cell-1", "clstm.cell0"):
        with pytest.raises(L.IvfError):
            gcv._clstm_layer(M, bad)
    with pytest.raises(L.IvfError):
        gcv._one_target(["clstm", "cell0"])
    with pytest.raises(L.IvfError):
        gcv._arch("VGG")


@pytest.mark.parametrize("entire", [0, 1])
@pytest.mark.parametrize("softmax", [0, 1])
def test_fixture_is_self_consistent(entire, softmax, golden):
    """The stored top-layer features and gradients reproduce the stored w, raw cam and final maps of target
    'clstm' and of target 'cell1' through the project's numpy restatement (oracle.gradcam_ref)."""
    from oracle import gradcam_ref
    g = golden("clstm_gradcam")
    feat = g["cell1_feat"]                                   # [T, hid, 7, 10]
    grad4 = g[f"e{entire}_s{softmax}_clstm_grad"]            # [4, hid, 7, 10]
    assert feat.shape == (T, 4, 7, 10) and grad4.shape == (4, 4, 7, 10)
    full = np.zeros_like(feat)
    full[EFF] = grad4                                        # what the top layer receives: endFC's gradient only
    for name, f, gr in (("clstm", feat[EFF], grad4), ("cell1", feat, full)):
        key = f"e{entire}_s{softmax}_{name}"
        for pf in (1, 0):
            vid, w, cam = gradcam_ref.cam_from_activations(f.transpose(1, 0, 2, 3), gr.transpose(1, 0, 2, 3), T, 160,
                                                           120, bool(pf))
            assert np.array_equal(w, g[key + "_w"]) and np.array_equal(cam, g[key + "_cam"])
            want = g[f"{key}_pf{pf}"]
            assert np.array_equal(vid[:, ::8, ::8] if pf else vid[::4, ::8, ::8], want)
            assert np.isfinite(want).all() and want.min() >= 0 and want.max() <= 1
    # the gradient reaches one effective step, or all four with use_entire_seq
    assert (np.abs(grad4).reshape(4, -1).max(axis=1) > 0).sum() == (4 if entire else 1)


def test_fixture_covers_every_case_and_has_no_nan(golden):
    g = golden("clstm_gradcam")
    for e in (0, 1):
        for s in (0, 1):
            for name in ("clstm", "cell0", "cell1"):
                key = f"e{e}_s{s}_{name}"
                for suffix in ("_pf1", "_pf0", "_probs", "_index", "_w", "_cam"):
                    assert np.isfinite(g[key + suffix]).all(), key + suffix
                assert g[key + "_pf1"].shape == (T, 15, 20) and g[key + "_pf0"].shape == (8, 15, 20)
                assert g[key + "_cam"].max() > 0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "clstm_gradcam.npz")) < 640 * 1024
