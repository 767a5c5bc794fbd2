"""CPU proof of tests/search_refs.py, on the inputs test_gpu_search_driver.py later runs the driver on: the float32 chain
meets the gate it defines, deliberately wrong chains do not, the free-running float64 loop keeps the ambiguity cap and
the pairing-threshold margin over its N_ITERS iterations, and the start masks hold the rows they are named for."""
import numpy as np
import pytest
import torch

import clstm_refs as CR
import search_refs as R
from conftest import note


@pytest.fixture(scope="module")
def runs():
    """(plan, mode) -> [(raw, measure)] of the free-running float64 loop, computed once"""
    cache = {}

    def get(pid, mode):
        if (pid, mode) not in cache:
            cache[pid, mode] = list(R.free_run(pid, mode))
        return cache[pid, mode]
    return get


@pytest.mark.parametrize("pid,mode", R.RUNS)
def test_float32_chain_meets_the_gate_and_the_caps_hold(pid, mode, runs):
    """per iteration of the float64 loop: every tensor of the float32 chain within GATE_MARGIN x its floor on every
    clip; at most ambiguous_cap clips with an ambiguous element (none but in P3); in reverse mode every sigmoid(raw) at
    least THRESH_MARGIN from 0.1f, so float32 and float64 pair the same frames"""
    plan = R.PLANS[pid]
    cap = R.ambiguous_cap(pid, plan.b)
    left = []
    for it, (raw, ms) in enumerate(runs(pid, mode)):
        e = R.errors(ms["f32"], ms["ref"])
        for n in R.TENSORS:
            assert ms["floor"][n] < 1e-3, f"{n}: a float32 floor of {ms['floor'][n]:.2e} is no float32-sized number"
            assert bool((e[n] <= ms["gate"][n]).all())
        left.append(int((ms["ambiguous"] > 0).sum()))
        assert left[-1] <= cap, f"iteration {it}: clips {np.nonzero(ms['ambiguous'])[0].tolist()} are ambiguous"
        if mode == "reverse":
            sig32 = torch.sigmoid(raw)
            assert float((sig32.double() - float(np.float32(0.1))).abs().min()) >= R.THRESH_MARGIN
            assert float(np.abs(ms["ref"]["sig"] - float(np.float32(0.1))).min()) >= R.THRESH_MARGIN
            assert np.array_equal(ms["ref"]["sig"] > R.THRESH, (sig32 > np.float32(0.1)).numpy())
        assert float(np.abs(ms["ref"]["dsig"]).max()) > 0
    fl = runs(pid, mode)[0][1]["floor"]
    note(f"search refs {pid} {mode}: float32 floors at the start " + " ".join(f"{n} {v:.2e}" for n, v in fl.items())
         + f"; clips left out per iteration {left} (cap {cap})")


@pytest.mark.parametrize("pid,mode,mutant", [(p, m, k) for p, m in R.RUNS for k in R.MUTANTS if R.mutant_applies(k, m)])
def test_mutants_land_outside_the_gate(pid, mode, mutant, runs):
    plan = R.PLANS[pid]
    x, net, targets = R.inputs(pid)
    assert len(set(targets[:plan.b])) >= 2
    raw, ms = runs(pid, mode)[0]
    bad = R.chain(pid, x[:plan.b], net, targets[:plan.b], raw, mode, torch.float64, mutant=mutant)
    e = R.errors(bad, ms["ref"])
    worst = {n: float(np.max(e[n] / ms["gate"][n])) for n in R.TENSORS}
    assert max(worst.values()) > 1.0, f"{R.MUTANTS[mutant]} stays inside every gate: {worst}"
    # (a) - (d) are wrong in the gradient or in what the network sees, not only in a number read off at the end
    if mutant != "logits" or plan.kind == "clstm":
        assert worst["dsig"] > 1.0 or worst["probs"] > 1.0


@pytest.mark.parametrize("pid", [p for p, m in R.RUNS if m == "reverse"])
def test_reverse_start_rows(pid):
    """every batch of at least three rows holds a row of each named kind; smaller batches begin with the mixed row; on
    the all-off row d score / d sig of the float64 chain is exactly 0.0"""
    plan = R.PLANS[pid]
    B, T = plan.case.B, plan.case.T
    assert T >= 3
    raw, on = R.rev_rows(pid, B, T)
    assert torch.equal(raw, R.start_raw(pid, "reverse", B, T))
    assert np.array_equal((torch.sigmoid(raw) > np.float32(0.1)).numpy(), on.numpy())
    for b in plan.sizes:
        props = set().union(*(R.rev_properties(on[r]) for r in range(b)))
        want = set(R.REV_PROPERTIES) if b >= 3 else {"even", "odd", "first", "last"}
        assert want <= props, f"b = {b}: no row with {sorted(want - props)}"
    assert R.rev_properties(on[0]) >= {"even", "odd", "first", "last"}
    x, net, targets = R.inputs(pid)
    if plan.b >= 2:
        assert R.rev_properties(on[1]) == {"all_off"}
        ref = R.chain(pid, x[:plan.b], net, targets[:plan.b], raw[:plan.b], "reverse")
        assert bool((ref["dsig"][1] == 0).all()) and float(np.abs(ref["dsig"][0]).max()) > 0
        assert float(R.reg_grad(torch.sigmoid(raw[1:2].double())).abs().min()) > 0      # the regulariser still moves it


def test_freeze_start_rows_are_distinct():
    for pid, plan in R.PLANS.items():
        raw = R.start_raw(pid, "freeze", plan.case.B, plan.case.T)
        assert len({tuple(r.tolist()) for r in raw}) == plan.case.B
        x, _, targets = R.inputs(pid)
        assert len({x[r].numpy().tobytes() for r in range(plan.case.B)}) == plan.case.B
        assert all(targets[r] != targets[r + 1] for r in range(plan.case.B - 1))


def test_eps_hat_is_formed_in_float32():
    """eps_hat32 against the double formula: equal to float32 accuracy, and far from eps itself at the first steps"""
    for step in (1, 2, 3, 1000):
        want = 1e-8 / np.sqrt(1.0 - 0.999 ** step)
        got = R.eps_hat32(1e-8, 0.999, step)
        assert abs(got - want) <= 1e-4 * want and got == float(np.float32(got))      # powf(beta2, step) near 1 cancels
    assert R.eps_hat32(1e-8, 0.999, 1) > 30e-8
    assert R.eps_at("S1", 1) == 1e-8 and R.eps_at("TF", 1) == R.eps_hat32(1e-8, 0.999, 1) and R.eps_at("TF", 1, plain=True) == 1e-8
    assert CR.GATE_MARGIN == 8.0 and CR.AMBIGUOUS_CAP == 1.0 / 16
