"""CPU proof of tests/clstm_refs.py on the case table the GPU test (test_gpu_clstm_kernels.py) runs: the float64
reference equals the oracle, the float32 floors, every mutant of the reference lands far outside the gate, the
recurrent weights matter, and the float64 reference meets the pool-ambiguity cap.  P cases run on their first 4
clips here (their ambiguity check on all 64, forward only)."""
import numpy as np
import pytest
import torch

import clstm_refs as CR
from oracle import clstm_ref

HOST_CLIPS = 4
_cache = {}


def _ref(cid):
    """The case's reference bundle on the clips the host tests use, computed once and left unchanged."""
    if cid not in _cache:
        case = CR.CASES[cid]
        _cache[cid] = CR.reference(case, min(case.b, HOST_CLIPS))
    return _cache[cid]


def _kept(bundle, name):
    """Clips that take part in the comparison of tensor `name`."""
    b = len(bundle["targets"])
    return [r for r in range(b) if not (CR.is_gradient(name) and r in bundle["left_out"])]


def _worst_ratio(bundle, res):
    """Largest err / gate over the compared tensors and clips of a (mutant) run, with the tensor it is on."""
    worst, where = 0.0, None
    for name, e in CR.errors(res, bundle["ref"]).items():
        kept = _kept(bundle, name)
        if kept and float(np.max(e[kept])) / bundle["gate"][name] > worst:
            worst, where = float(np.max(e[kept])) / bundle["gate"][name], name
    return worst, where


@pytest.mark.parametrize("cid", list(CR.CASES))
def test_reference_equals_oracle(cid):
    """probs to 1e-12 and dx against autograd of oracle.clstm_ref.forward, float64.  The oracle's use_entire_seq
    mixes the clips of a batch as the reference model does, so it is called one clip at a time."""
    case, bundle = CR.CASES[cid], _ref(cid)
    sd = {k: v.double() for k, v in bundle["sd"].items()}
    steps = case.out_steps if case.out_steps else (case.T - 1,)
    for r in range(len(bundle["targets"])):
        xr = bundle["x"][r:r + 1].double().requires_grad_()
        y = clstm_ref.forward(xr, sd, layers=case.layers, hidden=case.hid, kernel=case.k, stride=case.s,
                              steps=case.T, effective_step=steps, add_softmax=case.softmax,
                              batch_norm=case.batch_norm, use_entire_seq=case.out_steps is not None)
        assert np.max(np.abs(y.detach().numpy()[0] - bundle["ref"]["probs"][r])) < 1e-12
        if case.dout:
            (y * bundle["dout"][r:r + 1].double()).sum().backward()
        else:
            y[0, bundle["targets"][r]].backward()
        g = xr.grad.numpy()[0]
        assert np.max(np.abs(g - bundle["ref"]["dx"][r])) <= 1e-12 * max(1.0, float(np.max(np.abs(g))))


@pytest.mark.parametrize("cid", list(CR.CASES))
def test_floors(cid):
    """The float32 floor of every tensor (libm gates; for P cases also the persistent kernels' tanh form)."""
    bundle = _ref(cid)
    for variant, fl in bundle["variants"].items():
        print(f"[clstm floor] {cid} {variant}: " + " ".join(f"{n} {v:.2e}" for n, v in fl.items()))
    print(f"[clstm floor] {cid} gated on: " + " ".join(f"{n} {v:.2e}" for n, v in bundle["floor"].items()))
    for name, v in bundle["floor"].items():
        assert np.isfinite(v) and CR.U <= v < 1e-3, (name, v)      # a floor near the gates of old would gate nothing


@pytest.mark.parametrize("cid,mutant", [(c.id, m) for c in CR.CASES.values() for m in CR.MUTANTS
                                        if CR.mutant_applies(c, m, min(c.b, HOST_CLIPS))])
def test_mutant_exceeds_gate(cid, mutant):
    """Each wrong network is at least 10x the gate away on some compared tensor, on every case where it applies."""
    case, bundle = CR.CASES[cid], _ref(cid)
    res = CR.run(case, bundle["x"], bundle["sd"], torch.float64, mutant=mutant, targets=bundle["targets"],
                 dout=bundle["dout"])
    ratio, where = _worst_ratio(bundle, res)
    print(f"[clstm mutant] {cid} {mutant}: {ratio:.3g} x gate on {where}")
    assert ratio >= 10.0


def test_every_mutant_has_a_case():
    for mutant in CR.MUTANTS:
        assert any(CR.mutant_applies(c, mutant, min(c.b, HOST_CLIPS)) for c in CR.CASES.values()), mutant


@pytest.mark.parametrize("cid", [c.id for c in CR.CASES.values() if c.T >= 2])
def test_recurrence_matters(cid):
    """Zeroing every Wh moves the top layer's X by at least 100x its gate: the weights exercise the recurrence."""
    case, bundle = CR.CASES[cid], _ref(cid)
    res = CR.run(case, bundle["x"], bundle["sd"], torch.float64, mutant="nowh", backward=False)
    top = f"X{case.layers - 1}"
    ratio = float(np.max(CR.errors(res, bundle["ref"], forward_only=True)[top])) / bundle["gate"][top]
    print(f"[clstm recurrence] {cid}: {top} moves {ratio:.3g} x gate without Wh")
    assert ratio >= 100.0


@pytest.mark.parametrize("cid", list(CR.CASES))
def test_ambiguity_cap(cid):
    """The float64 reference alone meets the cap: S and W cases leave out no clip, P cases (all 64 clips, forward
    only) at most 1 in 16, and never the clip that is also run alone."""
    case = CR.CASES[cid]
    x, sd, _, _ = CR.case_inputs(case)
    ref = CR.run(case, x, sd, torch.float64, backward=False)
    fl, _ = CR.floors(case, x, sd, ref, backward=False)
    amb, ties = CR.ambiguous_windows(ref["pre"], fl)
    out = [int(r) for r in np.nonzero(amb)[0]]
    print(f"[clstm ambiguity] {cid}: {len(out)} of {len(amb)} clips left out {out}, exact ties {int(ties.sum())}")
    if case.path == "P":
        assert len(out) <= CR.AMBIGUOUS_CAP * len(amb)
        assert CR.SOLO_CLIP not in out
    else:
        assert not out
    assert (ties.sum() > 0) == case.tie       # exact ties where they were constructed, and nowhere else


def test_elem_err_measures_one_element_against_the_typical_size():
    r = np.ones((2, 1000))
    r[0, 0] = 1000.0
    a = r.copy()
    a[0, 5] += 0.1           # under max|r| this is 1e-4; against its own size it is 0.1 / (1 + rms)
    e = CR.elem_err(a, r)
    assert e[1] == 0.0 and 0.1 / (1 + 40) < e[0] < 0.1
    a[1, 3] = np.nan
    assert np.isnan(CR.elem_err(a, r)[1])
