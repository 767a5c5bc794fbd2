"""ConvLSTM kernels (csrc/convlstm.hip) against the per-layer float64 reference of tests/clstm_refs.py, one test
per case of its table: every dispatch family (stepwise split, persistent, wide), every template instance, and the
shapes at which each takes another branch.  Compared per clip and per element (clstm_refs.elem_err): probs, logits,
score, every layer's pooled output X[l], its gradient dX[l], and dx.  The gate is 8x the float32 floor of the same
tensor, measured here on the same inputs (DESIGN.md "ConvLSTM kernel gate"; test_clstm_refs_host.py proves on the
CPU that deliberately wrong networks land far outside it)."""
import os

import numpy as np
import pytest
import torch

import arena_fill as AF
import clstm_refs as CR
from conftest import note

pytestmark = pytest.mark.gpu


def _engine(case):
    import ivf_engine
    eng = ivf_engine.CLSTMEngine(CR.K, (case.C, case.T, case.H, case.W), max_batch=case.B, hidden=case.hid,
                                 layers=case.layers, kernel=case.k, stride=case.s, softmax=case.softmax,
                                 batch_norm=case.batch_norm,
                                 out_steps=list(case.out_steps) if case.out_steps else None)
    return eng


def _gpu_run(eng, case, x, targets, dout):
    """One forward and one backward of b = len(x) clips; the result in the layout of clstm_refs.run."""
    import ivf_lib as L
    b = x.shape[0]
    xg = x.cuda()
    probs, logits = eng.forward(xg, want_logits=True)
    # CLSTMEngine.backward with a dx of our own, NaN everywhere: whatever the plan leaves unwritten stays NaN.
    # This restates ivf_engine._Engine.backward (which allocates dx itself) and must track its argument order:
    # (handle, b, target, dout, score, dx, stream).
    C, T, H, W = eng.clip_shape
    dx = torch.full((b, C, T, H, W), float("nan"), device="cuda")
    tgt = eng._targets(targets, b) if dout is None else None
    dog = L.f32c(dout.cuda()) if dout is not None else None
    score = torch.empty(b, device="cuda") if tgt is not None else None
    L.check(eng._fn("backward")(eng._h, b, L.ptr(tgt), L.ptr(dog), L.ptr(score), L.ptr(dx), L.stream()))
    torch.cuda.synchronize()
    states = [eng.layer_state(l, b) for l in range(case.layers)]

    def np64(v):
        return v.detach().cpu().numpy().astype(np.float64)
    return {"probs": np64(probs), "logits": np64(logits), "score": None if score is None else np64(score),
            "X": [np64(s[0]) for s in states], "dX": [np64(s[1]) for s in states], "dx": np64(dx)}


def _check(case, bundle, res, label, clips_idx):
    """Every tensor of `res` (rows = the clips `clips_idx` of the bundle) against the float64 reference and the
    case's gate; figures are written before anything is asserted."""
    ref = {k: ([a[clips_idx] for a in v] if isinstance(v, list) else (None if v is None else v[clips_idx]))
           for k, v in bundle["ref"].items()}
    errs = CR.errors(res, ref)
    failures = []
    for name, e in errs.items():
        kept = [i for i, r in enumerate(clips_idx) if not (CR.is_gradient(name) and r in bundle["left_out"])]
        worst = float(np.max(e[kept])) if kept else 0.0
        fl, gate = bundle["floor"][name], bundle["gate"][name]
        note(f"clstm kernels {case.id} {label} {name}: floor {fl:.3e} gpu {worst:.3e} ratio {worst / fl:.2f} "
             f"(gate {CR.GATE_MARGIN:g}x, clips compared {len(kept)}/{len(clips_idx)})")
        if not worst <= gate:          # (NaN fails)
            bad = [clips_idx[i] for i in kept if not e[i] <= gate]
            failures.append(f"{name}: {worst:.3e} > gate {gate:.3e} (floor {fl:.3e}), clips {bad[:8]}")
    return failures


@pytest.mark.parametrize("cid", list(CR.CASES))
def test_clstm_case_matches_fp64_reference(cid):
    case = CR.CASES[cid]
    if case.path == "P" and "IVF_CLSTM_PERSIST" in os.environ:
        pytest.skip("IVF_CLSTM_PERSIST is set: the dispatch under test is overridden")
    bundle = CR.reference(case)
    if bundle["left_out"]:
        note(f"clstm kernels {case.id}: clips {bundle['left_out']} have an ambiguous pool window and are left out of "
             f"the gradient comparisons")
    assert len(bundle["left_out"]) <= (CR.AMBIGUOUS_CAP * case.b if case.path == "P" else 0)
    eng = _engine(case)
    eng.load_state_dict(bundle["sd"])
    res = _gpu_run(eng, case, bundle["x"], bundle["targets"], bundle["dout"])
    assert np.all(np.isfinite(res["dx"])), "dx has elements the backward never wrote"
    failures = _check(case, bundle, res, f"b={case.b}/B={case.B}", list(range(case.b)))
    if case.path == "P":
        # a clip's rows do not depend on its position or on the form of the recurrence: the same clip alone
        # (b = 1, stepwise kernels) meets the same gate
        r = CR.SOLO_CLIP
        solo = _gpu_run(eng, case, bundle["x"][r:r + 1], bundle["targets"][r:r + 1], None)
        assert np.all(np.isfinite(solo["dx"]))
        failures += _check(case, bundle, solo, f"clip {r} alone", [r])
    if cid == "S1":
        # the same gate on a plan whose arenas held 0xFF (NaN) when it was bound and loaded and whose workspace holds
        # it again before the forward: S1's unpool has to write the zeros of the dropped row itself
        # (test_gpu_arena_contents.py has the matrix)
        with AF.filled(0xFF):
            ff = _engine(case)
            ff.load_state_dict(bundle["sd"])
            AF.refill(ff, 0xFF)
            res = _gpu_run(ff, case, bundle["x"], bundle["targets"], bundle["dout"])
        assert np.all(np.isfinite(res["dx"])), "dx has elements the backward never wrote"
        failures += _check(case, bundle, res, f"b={case.b}/B={case.B} on 0xFF arenas", list(range(case.b)))
    assert not failures, "; ".join(failures)
