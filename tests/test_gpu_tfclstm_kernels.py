"""TF-style ConvLSTM kernels (csrc/tf_clstm.hip) against the per-layer float64 reference of tests/tfclstm_refs.py,
one test per case of its table: every stride, pad rule, kernel parity, map edge and batch edge at which a kernel
takes another branch.  Compared per clip and per element (clstm_refs.elem_err): every layer's output sequence H[l]
and pooled output X[l], logits, probs, score, every dX[l] and dx.  The gate is 8x the float32 floor of the same
tensor, measured on the same inputs (DESIGN.md "TF-style ConvLSTM kernel gate"; test_tfclstm_refs_host.py proves on
the CPU that deliberately wrong networks land outside it and that no clip has an ambiguous element).  Grad-CAM and
its resize are compared the same way with the float64 maps of tfclstm_refs.gradcam."""
import numpy as np
import pytest
import torch

import tfclstm_refs as TR
from conftest import note

pytestmark = pytest.mark.gpu

_engines = {}


def _engine(case, w=None):
    """The case's plan with its weights loaded (one per case, shared by the case test and the Grad-CAM tests)."""
    import ivf_engine
    if w is not None or case.id not in _engines:
        eng = ivf_engine.TFCLSTMEngine(TR.K, (case.C, case.T, case.H, case.W), units=case.units,
                                       kernel=(case.kh, case.kw), stride=case.s, padding=case.pad,
                                       recurrent_activation="hard_sigmoid" if case.hard else "sigmoid",
                                       only_last_element_for_fc=case.only_last, max_batch=case.B)
        assert eng.fc_inputs == TR.fc_inputs(case)
        for l, d in enumerate(TR.layer_dims(case)):
            assert eng.layer_dims(l) == (d[4], d[5], d[6], d[7], d[1])
        if w is not None:
            eng.load_weights(w["layers"], w["dense_w"], w["dense_b"])
            return eng
        w0 = TR.case_inputs(case)[1]
        eng.load_weights(w0["layers"], w0["dense_w"], w0["dense_b"])
        _engines[case.id] = eng
    return _engines[case.id]


def _gpu_run(eng, case, x, targets):
    """One forward and (unless the case is forward-only) one backward of b = len(x) clips; the result in the layout
    of tfclstm_refs.run.  The backward writes into a dx of the test's own, NaN everywhere: whatever the plan leaves
    unwritten stays NaN.  This restates TFCLSTMEngine.backward (which allocates dx itself) and must track its
    argument order: (handle, b, target, score, dx, stream)."""
    import ivf_lib as L
    b = x.shape[0]
    probs, logits = eng.forward(x.cuda(), want_logits=True)

    def np64(v):
        return v.detach().cpu().numpy().astype(np.float64)
    res = {"probs": np64(probs), "logits": np64(logits)}
    if not case.forward_only:
        C, T, H, W = eng.clip_shape
        dx = torch.full((b, C, T, H, W), float("nan"), device="cuda")
        tgt = eng._targets(targets, b)
        score = torch.empty(b, device="cuda")
        L.check(L.lib().ivf_tfclstm_backward(eng._h, b, L.ptr(tgt), L.ptr(score), L.ptr(dx), L.stream()))
        torch.cuda.synchronize()
        res["score"], res["dx"] = np64(score), np64(dx)
    states = [eng.layer_state(l, b) for l in range(len(case.units))]
    res["H"] = [np64(s[0]) for s in states]
    res["X"] = [np64(s[1]) for s in states]
    if not case.forward_only:
        res["dX"] = [np64(s[2]) for s in states]
    return res


def _check(case, bundle, res, label, clips_idx):
    """Every tensor of `res` (rows = the clips `clips_idx` of the bundle) against the float64 reference and the
    case's gate; figures are written before anything is asserted."""
    ref = {k: ([a[clips_idx] for a in v] if isinstance(v, list) else v[clips_idx]) for k, v in bundle["ref"].items()}
    failures = []
    for name, e in TR.errors(res, ref, case.forward_only).items():
        worst = float(np.max(e))
        fl, gate = bundle["floor"][name], bundle["gate"][name]
        note(f"tfclstm kernels {case.id} {label} {name}: floor {fl:.3e} gpu {worst:.3e} ratio {worst / fl:.2f} "
             f"(gate {TR.GATE_MARGIN:g}x, clips compared {len(clips_idx)}/{len(clips_idx)})")
        if not worst <= gate:          # (NaN fails)
            bad = [clips_idx[i] for i in range(len(clips_idx)) if not e[i] <= gate]
            failures.append(f"{name}: {worst:.3e} > gate {gate:.3e} (floor {fl:.3e}), clips {bad[:8]}")
    return failures


@pytest.mark.parametrize("cid", list(TR.CASES))
def test_tfclstm_case_matches_fp64_reference(cid):
    case = TR.CASES[cid]
    bundle = TR.reference(case)
    if not case.forward_only:
        assert not bundle["left_out"]              # the cap is zero clips: every clip is compared on every tensor
    eng = _engine(case)
    res = _gpu_run(eng, case, bundle["x"], bundle["targets"])
    if not case.forward_only:
        assert np.all(np.isfinite(res["dx"])), "dx has elements the backward never wrote"
    for v in res["H"] + res["X"] + res.get("dX", []):
        assert np.all(np.isfinite(v))
    failures = _check(case, bundle, res, f"b={case.b}/B={case.B}", list(range(case.b)))
    if cid == "A":
        # a clip's rows do not depend on its position in the batch: clip 2 alone (b = 1) meets the same gate
        solo = _gpu_run(eng, case, bundle["x"][2:3], bundle["targets"][2:3])
        assert np.all(np.isfinite(solo["dx"]))
        failures += _check(case, bundle, solo, "clip 2 alone", [2])
    if cid == "C":
        # stride 3 'valid' on 20 x 27 reads rows 0..17 and columns 0..25: the rest of dx is written, and exactly 0
        assert np.all(res["dx"][..., 18:, :] == 0.0) and np.all(res["dx"][..., 26] == 0.0)
        assert np.any(res["dx"][..., 17, :26] != 0.0)
    assert not failures, "; ".join(failures)


def _cam_check(tag, got, want, gate, floor):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{tag}: NaN pattern differs"
    worst = float(np.max(TR.cam_err(got, want)))
    note(f"tfclstm kernels {tag}: floor {floor:.3e} gpu {worst:.3e} ratio {worst / floor:.2f} (gate {TR.GATE_MARGIN:g}x)")
    return [] if worst <= gate else [f"{tag}: {worst:.3e} > gate {gate:.3e}"]


@pytest.mark.parametrize("cid,out_hw", TR.CAM_RUNS)
def test_tfclstm_gradcam_matches_fp64_reference(cid, out_hw):
    """tf_gradcam_kernel and tf_cam_resize_kernel, both normalisation modes, against the float64 maps: identical NaN
    pattern (a frame that receives no gradient is 0/0 in 'frame' mode), the rest inside 8x the float32 floor."""
    case = TR.CASES[cid]
    g = TR.gradcam_reference(case, out_hw)
    assert g["nan_equal"] and not g["ambiguous_frames"].any()
    eng = _engine(case)
    failures = []
    for mode in ("frame", "sequence"):
        cam, _ = eng.gradcam(g["x"].cuda(), g["targets"], normalization_mode=mode, out_hw=out_hw)
        assert tuple(cam.shape[2:]) == (out_hw if out_hw is not None else (case.H, case.W))
        failures += _cam_check(f"{cid} gradcam {mode} {tuple(cam.shape[2:])}", cam, g["ref"][mode], g["gate"][mode],
                               g["floor"][mode])
    assert not failures, "; ".join(failures)


def test_tfclstm_gradcam_of_a_class_without_dense_weights_is_nan_per_frame():
    """Constructed edge: with the dense kernel's entries of the target class zeroed no gradient reaches any frame, so
    every frame is 0/0: 'frame' mode returns NaN everywhere (and so does 'sequence': the sequence maximum is 0)."""
    case = TR.CASES["A"]
    x, w, targets = TR.case_inputs(case)
    w = dict(w, dense_w=w["dense_w"].clone())
    for t in set(targets):
        w["dense_w"][:, t] = 0.0
    want = TR.gradcam(case, x, w, targets)
    assert np.isnan(want["frame"]).all() and np.isnan(want["sequence"]).all()
    eng = _engine(case, w)
    for mode in ("frame", "sequence"):
        cam, _ = eng.gradcam(x.cuda(), targets, normalization_mode=mode)
        assert bool(torch.isnan(cam).all()), mode
