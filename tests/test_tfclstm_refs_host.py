"""CPU proof of tests/tfclstm_refs.py on the case table the GPU test (test_gpu_tfclstm_kernels.py) runs: the float32
run equals the oracle, the float32 floors are finite, the float64 reference has no ambiguous element (zero-clip cap,
pool windows and hard-sigmoid kinks), case G is saturated, case S has exact ties and nothing else, the Grad-CAM
inputs have no ambiguous frame, and every mutant of the reference lands outside the gate on every case it applies
to."""
import numpy as np
import pytest
import torch

import tfclstm_refs as TR
from oracle import tfclstm_ref

_cache = {}
_cam_cache = {}

CAM_RUNS = TR.CAM_RUNS


def _ref(cid):
    """The case's reference bundle, computed once and left unchanged."""
    if cid not in _cache:
        _cache[cid] = TR.reference(TR.CASES[cid])
    return _cache[cid]


def _worst_ratio(bundle, res):
    """Largest err / gate over the compared tensors and clips of a (mutant) run, with the tensor it is on."""
    worst, where = 0.0, None
    for name, e in TR.errors(res, bundle["ref"]).items():
        r = float(np.max(e)) / bundle["gate"][name]
        if not r <= worst:          # (NaN counts as outside)
            worst, where = r, name
    return worst, where


@pytest.mark.parametrize("cid", list(TR.CASES))
def test_float32_run_equals_oracle(cid):
    """Where the two overlap (logits, the last block's output sequence, dx of the scores): the float32 run of the
    restatement against oracle.tfclstm_ref.model, the same operations in the same order, so to a few roundings of
    the tensor's size (the hand-written pool and the batched x-convolution may reorder nothing but the backward sums)."""
    case = TR.CASES[cid]
    x, w, targets = TR.case_inputs(case)
    res = TR.run(case, x, w, torch.float32, targets=targets, backward=not case.forward_only)
    xr = x.clone().requires_grad_(not case.forward_only)
    lg, last = tfclstm_ref.model(xr, w, stride=case.s, padding=case.pad, hard=case.hard, only_last=case.only_last)

    def close(a, r, what):
        r = np.asarray(r, np.float64)
        assert np.max(np.abs(a - r)) <= 16 * TR.U * max(1.0, float(np.max(np.abs(r)))), what
    close(res["logits"], lg.detach().numpy(), "logits")
    close(res["H"][-1], last.detach().numpy(), "last output sequence")
    if not case.forward_only:
        pr = torch.softmax(lg, 1)
        pr[torch.arange(len(targets)), torch.as_tensor(targets)].sum().backward()
        close(res["dx"], xr.grad.numpy(), "dx")
    # the geometry of the restatement is the table's
    for l, d in enumerate(TR.layer_dims(case)):
        assert res["H"][l].shape[2:] == (d[1], d[4], d[5]) and res["X"][l].shape[2:] == (d[1], d[6], d[7])
        assert d[6] >= 1 and d[7] >= 1 and d[4] >= 2 and d[5] >= 2


@pytest.mark.parametrize("cid", list(TR.CASES))
def test_floors(cid):
    bundle = _ref(cid)
    print(f"[tfclstm floor] {cid}: " + " ".join(f"{n} {v:.2e}" for n, v in bundle["floor"].items()))
    case = TR.CASES[cid]
    names = list(bundle["floor"])
    assert ("dx" in names) == (not case.forward_only)
    for l in range(len(case.units)):
        assert f"H{l}" in names and f"X{l}" in names and ((f"dX{l}" in names) == (not case.forward_only))
    for name, v in bundle["floor"].items():
        assert np.isfinite(v) and TR.U <= v < 1e-4, (name, v)      # a floor near the gates of old would gate nothing


@pytest.mark.parametrize("cid", [c.id for c in TR.CASES.values() if not c.forward_only])
def test_zero_clip_cap(cid):
    """The float64 reference alone has no ambiguous pool window and no gate pre-activation at the hard-sigmoid kink:
    no clip of any case is left out of the gradient comparisons.  Exact ties are structural and counted apart:
    constructed in S; in G where the output gate is clamped to exactly 0 (the tied maximum is 0 and no gradient
    passes a clamped gate); nowhere else."""
    case, bundle = TR.CASES[cid], _ref(cid)
    print(f"[tfclstm ambiguity] {cid}: pool {bundle['pool_ambiguous'].tolist()} kink {bundle['kink_ambiguous'].tolist()} "
          f"exact ties {bundle['ties'].tolist()} saturated {bundle['saturated'].tolist()}")
    assert not bundle["pool_ambiguous"].any()
    assert not bundle["kink_ambiguous"].any()
    assert not bundle["left_out"]
    if case.tie:
        assert bundle["ties"].min() > 0
    elif cid == "G":
        for v in bundle["ref"]["H"]:
            Hp, Wp = v.shape[-2] // 2, v.shape[-1] // 2
            v = v[..., :2 * Hp, :2 * Wp]
            c = np.sort(np.stack([v[..., 0::2, 0::2], v[..., 0::2, 1::2], v[..., 1::2, 0::2], v[..., 1::2, 1::2]], -1), -1)
            tied = c[..., 3] == c[..., 2]
            assert np.all(c[..., 3][tied] == 0.0)
    else:
        assert bundle["ties"].sum() == 0


def test_nokink_cases_are_the_saturated_ones():
    got = tuple(c.id for c in TR.CASES.values() if not c.forward_only and c.hard and _ref(c.id)["saturated"].sum() > 0)
    assert got == TR.NOKINK_CASES


def test_case_g_is_saturated():
    """In each layer of G, between 10 % and 90 % of the recurrent-gate pre-activations lie beyond the kink."""
    shares = TR.saturated_share(_ref("G")["ref"]["z"])
    print("[tfclstm saturation] G: " + " ".join(f"layer {l} {v:.1%}" for l, v in enumerate(shares)))
    assert len(shares) == 2 and all(0.10 <= v <= 0.90 for v in shares)


def test_case_c_reference_leaves_unread_input_at_zero():
    dx = _ref("C")["ref"]["dx"]
    assert np.all(dx[..., 18:, :] == 0) and np.all(dx[..., 26] == 0) and np.any(dx[..., 17, :26] != 0)


def test_case_i_takes_a_second_grid_stride_trip():
    case = TR.CASES["I"]
    _, Fu, _, _, Ho, Wo, _, _ = TR.layer_dims(case)[0]
    assert case.b * case.T * Fu * Ho * Wo > 16384 * 256


@pytest.mark.parametrize("cid,mutant", [(c.id, m) for c in TR.CASES.values() for m in TR.MUTANTS
                                        if TR.mutant_applies(c, m)])
def test_mutant_exceeds_gate(cid, mutant):
    case, bundle = TR.CASES[cid], _ref(cid)
    res = TR.run(case, bundle["x"], bundle["w"], torch.float64, mutant=mutant, targets=bundle["targets"])
    ratio, where = _worst_ratio(bundle, res)
    print(f"[tfclstm mutant] {cid} {mutant}: {ratio:.3g} x gate on {where}")
    assert ratio > 1.0


def test_every_mutant_has_a_case():
    for mutant in TR.MUTANTS:
        assert any(TR.mutant_applies(c, mutant) for c in TR.CASES.values()), mutant
    assert [c.id for c in TR.CASES.values() if TR.mutant_applies(c, "gateorder")] == \
        [c.id for c in TR.CASES.values() if not c.forward_only]


def _cam(cid, out_hw):
    if (cid, out_hw) not in _cam_cache:
        _cam_cache[(cid, out_hw)] = TR.gradcam_reference(TR.CASES[cid], out_hw)
    return _cam_cache[(cid, out_hw)]


@pytest.mark.parametrize("cid,out_hw", CAM_RUNS)
def test_gradcam_inputs_have_no_ambiguous_frame(cid, out_hw):
    """The float32 run has the float64 run's NaN pattern, its floor is finite, no frame's maximum sits within tau of
    zero, and the float64 restatement equals the oracle's float32 Grad-CAM to float32 accuracy."""
    case, g = TR.CASES[cid], _cam(cid, out_hw)
    print(f"[tfclstm gradcam floor] {cid} {out_hw}: " + " ".join(f"{m} {v:.2e}" for m, v in g["floor"].items()))
    assert g["nan_equal"] and not g["ambiguous_frames"].any()
    assert all(np.isfinite(v) and v < 1e-4 for v in g["floor"].values())
    assert np.isfinite(g["ref"]["sequence"]).all()
    kw = dict(stride=case.s, padding=case.pad, hard=case.hard, only_last=case.only_last)
    for mode in ("frame", "sequence"):
        want, _ = tfclstm_ref.gradcam_frames(g["x"][:1], g["w"], g["targets"][0], per_frame=(mode == "frame"),
                                             out_hw=out_hw, **kw)
        assert np.array_equal(np.isnan(want), np.isnan(g["ref"][mode][0]))
        assert float(TR.cam_err(want[None], g["ref"][mode][:1])[0]) < 1e-4


def test_resize_is_the_identity_at_equal_size_and_exact_on_a_ramp():
    a = np.arange(12, dtype=np.float64).reshape(3, 4)
    assert np.array_equal(TR.resize_bilinear(a, 3, 4), a)
    up = TR.resize_bilinear(a, 6, 8)
    assert up.shape == (6, 8) and up[0, 0] == 0 and up[-1, -1] == 11
    assert np.allclose(np.diff(up[2, 1:-1]), 0.5)          # interior of a ramp: half a source step per pixel
