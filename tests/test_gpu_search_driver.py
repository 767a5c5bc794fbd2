"""The temporal mask search driver (csrc/search_driver.h, run_search; ivf_i3d_search, ivf_clstm_search,
ivf_tfclstm_search) pinned to its pieces and to float64, batched (tests/search_refs.py: plans, start masks, the chain
reference and its gate; tests/test_search_refs_host.py proves them on the CPU on the same inputs).

1. Driver == pieces.  N = 3 iterations are replayed through the public entries run_search itself calls, in its order:
   ivf_mask_reg, the staging piece (ivf_freeze_fwd, or ivf_submask_pairs_batched + ivf_reverse_fwd_batched), the plan's
   forward and backward, ivf_freeze_bwd / ivf_reverse_bwd, ivf_search_step.  On I3D the clip is staged into
   ivf_i3d_input_buffer and the mask backward reads ivf_i3d_input_grad_buffer (16-byte channels-last pixels); on the
   ConvLSTM plans both are NCTHW tensors.  After every iteration raw_mask, exp_avg, exp_avg_sq and the trajectory row
   equal the driver's as int32 bits; the driver runs as 3, as 1 + 2 and as 1 + 1 + 1 through `state`.  The pairing rows
   of reverse mode are the replay's own tensors: the driver keeps its in plan scratch that has no public address.
2. On the ConvLSTM and TF plans the pieces' sig, probs, score and d score / d sig of every iteration are compared with
   the float64 chain of search_refs on the GPU's own raw of that iteration, at GATE_MARGIN x the float32 floor measured
   on the same raw on the CPU.
3. On I3D the plan's own input gradient goes through the mask backward: d score / d sig against
   mask_refs.freeze_bwd_ref / leaf_refs.reverse_bwd_ref on the buffer read back, at their own bounds (a whole-chain
   float64 autograd is not meaningful there: ReLU and arg-max gates flip, see test_gpu_i3d_small.py).

Every bit-for-bit assertion below held as written on the MI355X; no exception had to be documented."""
import time
from collections import namedtuple

import numpy as np
import pytest
import torch

import clstm_refs as CR
import i3d_refs as IR
import leaf_refs as LR
import mask_refs
import search_refs as R
from conftest import note
from test_gpu_leaf_kernels import bits, guarded, inside, untouched  # noqa: F401
from test_gpu_mask_kernels import NAN_BITS
from test_gpu_stmask import nan_guarded

pytestmark = pytest.mark.gpu

_T0 = []
N = R.N_ITERS
SPLITS = ([N], [1, N - 1], [1] * N)
ODD16 = IR.Case("odd16", (3, 16, 33, 47), dict(head_hw=(2, 2)), ("fp32",))      # `odd` with T = 16: the <16> cl4 scans
I3D_PLANS = [("odd", "fp32"), ("smod", "fp32"), ("gray", "fp32"), ("odd", "bf16act"), ("odd16", "fp32")]
I3D_TARGETS = [1, 4, 2]

Setup = namedtuple("Setup", "label pc x targets B modes sizes pid")


# ---------------------------------------------------------------------------------------------------- the pieces
class Pieces:
    """The public entries run_search calls, on the buffers it uses.  layout: 0 NCTHW, 4 16-byte channels-last pixels."""
    layout = 0

    def __init__(self, eng):
        self.eng = eng
        self.C, self.T, H, W = eng.clip_shape
        self.HW = H * W
        self.partner = None

    def stage(self, x, sig, b, mode):
        import ivf_lib as L
        dst = self.stage_buffer()
        if mode == "freeze":
            L.check(L.lib().ivf_freeze_fwd(L.ptr(x), L.ptr(sig), L.ptr(dst), b, self.C, self.T, self.HW, 1, self.layout, L.stream()))
            return
        self.partner = torch.empty(b, self.T, dtype=torch.int32, device="cuda")
        weight = torch.empty(b, self.T, device="cuda")
        L.check(L.lib().ivf_submask_pairs_batched(L.ptr(sig), b, self.T, 0.1, L.ptr(self.partner), L.ptr(weight), L.stream()))
        L.check(L.lib().ivf_reverse_fwd_batched(L.ptr(x), L.ptr(self.partner), L.ptr(weight), L.ptr(dst), b, self.C, self.T,
                                                self.HW, self.layout, L.stream()))

    def mask_bwd(self, x, sig, din, b, mode):
        """d score / d sig [b,T] of the staged clip's gradient `din`, into a NaN-filled buffer with sentinel rows"""
        import ivf_lib as L
        buf, dsig = nan_guarded((b, self.T))
        ws = torch.empty(L.lib().ivf_freeze_bwd_workspace_bytes(b, self.T), dtype=torch.uint8, device="cuda")
        if mode == "freeze":
            L.check(L.lib().ivf_freeze_bwd(L.ptr(x), L.ptr(sig), L.ptr(din), L.ptr(dsig), None, b, self.C, self.T, self.HW, 1,
                                           self.layout, L.ptr(ws), L.stream()))
        else:
            L.check(L.lib().ivf_reverse_bwd(L.ptr(x), L.ptr(self.partner), L.ptr(din), L.ptr(dsig), b, self.C, self.T, self.HW,
                                            self.layout, L.ptr(ws), L.stream()))
        torch.cuda.synchronize()
        assert untouched(buf), "mask backward: a sentinel row was written"
        assert not bool(torch.isnan(dsig).any()), "mask backward: an entry was never written"
        return dsig


class I3DPieces(Pieces):
    layout = 4

    def __init__(self, eng):
        import ivf_lib as L
        super().__init__(eng)
        self.inbuf = self._view(L.lib().ivf_i3d_input_buffer(eng._h))
        self.dinbuf = self._view(L.lib().ivf_i3d_input_grad_buffer(eng._h))

    def _view(self, p):
        eng = self.eng
        off = p - eng._ws.data_ptr()
        n = eng.max_batch * self.T * self.HW * 4
        assert 0 <= off and off + 4 * n <= eng._ws.numel()
        return eng._ws[off:off + 4 * n].view(torch.float32).view(eng.max_batch, self.T, self.HW, 4)

    def stage_buffer(self):
        return self.inbuf

    def forward(self, b):
        import ivf_lib as L
        probs = torch.empty(b, self.eng.K, device="cuda")
        L.check(L.lib().ivf_i3d_forward_staged(self.eng._h, b, None, L.ptr(probs), L.stream()))
        return probs

    def backward(self, b, tgt):
        import ivf_lib as L
        score = torch.empty(b, device="cuda")
        L.check(L.lib().ivf_i3d_backward(self.eng._h, b, L.ptr(tgt), None, L.ptr(score), None, L.stream()))      # dx = NULL
        return score, self.dinbuf[:b]


class SeqPieces(Pieces):
    """ConvLSTM and TF ConvLSTM: the clip is staged NCTHW, forward and backward are the engine's"""

    def __init__(self, eng):
        super().__init__(eng)
        self.P = torch.empty((eng.max_batch,) + tuple(eng.clip_shape), device="cuda")

    def stage_buffer(self):
        return self.P

    def forward(self, b):
        return self.eng.forward(self.P[:b])

    def backward(self, b, tgt):
        score, dx = self.eng.backward(b, tgt)[:2]
        return score, dx


# ---------------------------------------------------------------------------------------------------- plans
_SETUPS = {}


def i3d_setup(cid, math):
    import ivf_engine
    from test_gpu_i3d_small import engine
    key = ("i3d", cid, math)
    if key not in _SETUPS:
        if cid == "odd16":
            eng = ivf_engine.I3DEngine(IR.NUM_CLASSES, ODD16.clip, max_batch=IR.MAX_BATCH, softmax=True, math=math, **ODD16.engine)
            eng.load_state_dict(IR.state_dict(ODD16), autotune=False)
            case = ODD16
        else:
            eng, case = engine(cid, math), IR.CASES[cid]
        x = IR.clips(case).cuda().contiguous()
        assert len({x[r].cpu().numpy().tobytes() for r in range(IR.MAX_BATCH)}) == IR.MAX_BATCH
        tg = torch.tensor(I3D_TARGETS, dtype=torch.int32, device="cuda")
        _SETUPS[key] = Setup(f"i3d {cid} {math}", I3DPieces(eng), x, tg, IR.MAX_BATCH, R.MODES, (1, 2, 3), f"i3d_{cid}")
    return _SETUPS[key]


def seq_setup(pid):
    key = ("seq", pid)
    if key not in _SETUPS:
        plan = R.PLANS[pid]
        x, net, targets = R.inputs(pid)
        if plan.kind == "clstm":
            from test_gpu_clstm_kernels import _engine
            eng = _engine(plan.case)
            eng.load_state_dict(net)
        else:
            from test_gpu_tfclstm import _setup
            eng, w, _, _ = _setup(B=plan.case.B)
            for mine, theirs in zip(net["layers"], w["layers"]):          # the plan of test_gpu_tfclstm.py, weights and all
                assert all(torch.equal(p, q) for p, q in zip(mine, theirs))
            assert torch.equal(net["dense_w"], w["dense_w"]) and tuple(eng.clip_shape) == tuple(x.shape[1:])
        tg = torch.tensor(targets, dtype=torch.int32, device="cuda")
        _SETUPS[key] = Setup(f"{plan.kind} {pid}", SeqPieces(eng), x.cuda().contiguous(), tg, plan.case.B, plan.modes, plan.sizes, pid)
    return _SETUPS[key]


def setup_of(key):
    _T0.append(time.time())
    return i3d_setup(*key[1:]) if key[0] == "i3d" else seq_setup(key[1])


ALL_PLANS = [("i3d",) + p for p in I3D_PLANS] + [("seq", pid) for pid in R.PLANS]
PLAN_MODES = [(k, m) for k in ALL_PLANS for m in (R.MODES if k[0] == "i3d" else R.PLANS[k[1]].modes)]


def _id(v):
    return "-".join(v) if isinstance(v, tuple) else str(v)


def start(su, mode, b):
    return R.start_raw(su.pid, mode, su.B, su.pc.T)[:b].cuda().contiguous()


# ---------------------------------------------------------------------------------------------------- driver and replay
class State:
    """raw, exp_avg, exp_avg_sq of b clips as the leading rows of NaN-filled [B,T] buffers with sentinel rows around"""

    def __init__(self, B, raw0):
        b, T = raw0.shape
        self.b = b
        self.bufs, self.body = zip(*(nan_guarded((B, T)) for _ in range(3)))
        self.raw, self.m, self.v = (t[:b] for t in self.body)
        self.raw.copy_(raw0)
        self.m.zero_()
        self.v.zero_()

    def check_guards(self, what):
        torch.cuda.synchronize()
        for buf, body in zip(self.bufs, self.body):
            assert untouched(buf), f"{what}: a sentinel row of raw / exp_avg / exp_avg_sq was written"
            assert bool((bits(body[self.b:]) == NAN_BITS).all()), f"{what}: a row >= b was written"
            assert not bool(torch.isnan(body[:self.b]).any())

    def snapshot(self):
        return tuple(t.clone() for t in (self.raw, self.m, self.v))


def traj_rows(n, b):
    return nan_guarded((n, b, 4))


def check_traj(buf, traj, what):
    torch.cuda.synchronize()
    assert untouched(buf), f"{what}: a sentinel row of the trajectory was written"
    assert not bool(torch.isnan(traj).any()), f"{what}: a trajectory row was never written"


def drive(su, x, tgt, raw0, mode, parts, after_call=None):
    """ivf_<plan>_search on guarded buffers, `parts` iterations per call continued through first_step.  Returns the
    states after every call [(raw, m, v)] and the trajectory rows [sum(parts), b, 4]."""
    import ivf_lib as L
    eng = su.pc.eng
    b = raw0.shape[0]
    st = State(su.B, raw0)
    a = R.ADAM
    states, rows, done = [], [], 0
    for n in parts:
        tb, traj = traj_rows(n, b)
        L.check(eng._fn("search")(eng._h, L.ptr(x), b, L.ptr(tgt), L.ptr(st.raw), L.ptr(st.m), L.ptr(st.v), R.LAM1, R.LAM2,
                                  a["lr"], a["b1"], a["b2"], a["eps"], n, done + 1, *eng._mode_args(mode), L.ptr(traj), L.stream()))
        done += n
        st.check_guards(f"{su.label} driver {parts}")
        check_traj(tb, traj, f"{su.label} driver {parts}")
        states.append(st.snapshot())
        rows.append(traj.clone())
        if after_call is not None:
            after_call(len(states))
    return states, torch.cat(rows, 0)


def replay(su, x, tgt, raw0, mode, n=N, plain_eps=False, observe=None, lam1=R.LAM1):
    """n iterations by the pieces.  Returns the states after every iteration, the trajectory rows, and per iteration a
    record of what the pieces produced: raw (before the step), sig, probs, score, dsig."""
    import ivf_lib as L
    pc = su.pc
    b, T = raw0.shape
    st = State(su.B, raw0)
    a = R.ADAM
    states, rows, recs = [], [], []
    for step in range(1, n + 1):
        rec = {"raw": st.raw.clone()}
        sig, terms, dreg = torch.empty(b, T, device="cuda"), torch.empty(b, 2, device="cuda"), torch.empty(b, T, device="cuda")
        L.check(L.lib().ivf_mask_reg(L.ptr(st.raw), b, T, lam1, R.LAM2, L.ptr(sig), L.ptr(terms), L.ptr(dreg), L.stream()))
        pc.stage(x, sig, b, mode)
        probs = pc.forward(b)
        score, din = pc.backward(b, tgt)
        dsig = pc.mask_bwd(x, sig, din, b, mode)
        rec.update(sig=sig, probs=probs, score=score, dsig=dsig, dreg=dreg)
        if observe is not None:
            observe(step, rec, din)
        tb, trow = traj_rows(1, b)
        L.check(L.lib().ivf_search_step(L.ptr(st.raw), L.ptr(sig), L.ptr(dsig), L.ptr(dreg), L.ptr(terms), L.ptr(score),
                                        L.ptr(st.m), L.ptr(st.v), L.ptr(trow), b, T, step, a["lr"], a["b1"], a["b2"],
                                        R.eps_at(su.pid, step, plain=plain_eps), L.stream()))
        st.check_guards(f"{su.label} replay")
        check_traj(tb, trow, f"{su.label} replay")
        states.append(st.snapshot())
        rows.append(trow.clone())
        recs.append(rec)
    return states, torch.cat(rows, 0), recs


def same(p, q):
    return torch.equal(bits(p), bits(q))


_RUNS = {}


def both(su, mode, b, observe=None):
    """driver (every split) and replay of a (plan, mode, b), asserted equal bit for bit, computed once"""
    key = (su.label, mode, b, observe is not None)
    if key in _RUNS:
        return _RUNS[key]
    x, tgt, raw0 = su.x[:b], su.targets[:b].contiguous(), start(su, mode, b)
    what = f"{su.label} {mode} b={b}/B={su.B}"
    din1 = []

    def after_call(k):
        if k == 1 and su.pc.layout == 4:
            din1.append(su.pc.eng.endpoint("input:grad", b))
    driven = [drive(su, x, tgt, raw0, mode, parts, after_call if parts == SPLITS[-1] else None) for parts in SPLITS]
    states, rows, recs = replay(su, x, tgt, raw0, mode, observe=observe)
    for parts, (dst, drows) in zip(SPLITS, driven):
        for name, p, q in zip(("raw_mask", "exp_avg", "exp_avg_sq"), dst[-1], states[-1]):
            assert same(p, q), f"{what}: {name} after {N} iterations, driver as {parts}, differs from the pieces"
        assert same(drows, rows), f"{what}: trajectory of the driver as {parts} differs from the pieces"
    one = driven[0][0][0]
    first = driven[1][0][0]
    for k, (dst, mine) in enumerate(zip(driven[2][0], states)):               # after EVERY iteration
        for name, p, q in zip(("raw_mask", "exp_avg", "exp_avg_sq"), dst, mine):
            assert same(p, q), f"{what}: {name} after iteration {k + 1} differs from the pieces"
    assert all(same(p, q) for p, q in zip(first, states[0])) and all(same(p, q) for p, q in zip(one, states[-1]))
    assert not same(states[-1][0], raw0) and bool(torch.isfinite(rows).all())
    _RUNS[key] = dict(states=states, rows=rows, recs=recs, din1=din1[0] if din1 else None, raw0=raw0)
    return _RUNS[key]


# ---------------------------------------------------------------------------------------------------- 1. driver == pieces
@pytest.mark.parametrize("key,mode", PLAN_MODES, ids=_id)
def test_driver_equals_its_pieces(key, mode):
    """every batch size of the plan: b = 1, 1 < b < B and b = B where it has them (P3: b = B = 64, the persistent
    recurrence).  On the all-off row of a reverse batch d score / d sig is exactly 0.0 and the regulariser alone
    moves the mask."""
    su = setup_of(key)
    for b in su.sizes:
        res = both(su, mode, b)
        if mode == "reverse":
            on = R.rev_rows(su.pid, su.B, su.pc.T)[1][:b]
            for rec in res["recs"]:
                sig = rec["sig"].cpu()
                assert float((sig.double() - float(np.float32(0.1))).abs().min()) >= R.THRESH_MARGIN
                assert torch.equal(sig > np.float32(0.1), on), f"{su.label}: the runs changed within {N} iterations"
                off = ~on.any(1)
                assert bool((bits(rec["dsig"].cpu()[off]) == 0).all()), f"{su.label}: d score / d sig of an all-off row is not +0.0"
            if b >= 2:
                assert not bool(on[1].any()) and not same(res["states"][-1][0][1], res["raw0"][1])
        else:
            for rec in res["recs"]:
                assert bool((bits(rec["dsig"][:, 0]) == 0).all()), f"{su.label}: d score / d sig of frame 0 is not +0.0"


@pytest.mark.parametrize("key,mode", PLAN_MODES, ids=_id)
def test_perturbed_forward_equals_staging_plus_forward(key, mode):
    """eng.perturbed_forward (the init_mask path) at b < B, bit for bit"""
    su = setup_of(key)
    sizes = [b for b in su.sizes if b < su.B]
    if not sizes:
        assert key == ("seq", "P3")          # b = B = 64 is the only batch of the persistent case
        sizes = [su.B]
    b = sizes[-1]
    x = su.x[:b]
    mask = torch.sigmoid(start(su, mode, b))
    eng = su.pc.eng
    got = eng.perturbed_forward(x, mask, mode) if eng._has_mode else eng.perturbed_forward(x, mask)
    su.pc.stage(x, mask, b, mode)
    want = su.pc.forward(b)
    torch.cuda.synchronize()
    assert same(got, want), f"{su.label} {mode} b={b}: perturbed_forward differs from the staging piece + forward"
    assert float((got - eng.forward(x)).abs().max()) > 0, "the perturbation does not reach the network"


@pytest.mark.parametrize("key,mode", PLAN_MODES, ids=_id)
def test_rows_do_not_depend_on_the_batch(key, mode):
    """the driver on a permuted batch gives the permuted rows; a clip searched alone (b = 1) reproduces its rows.  P3 has
    the permutation only: alone, a clip runs the stepwise recurrence, whose arithmetic differs by design."""
    su = setup_of(key)
    b = su.sizes[-1]
    raw0 = start(su, mode, b)
    tgt = su.targets[:b].contiguous()
    base_s, base_r = drive(su, su.x[:b], tgt, raw0, mode, [N])
    perm = torch.roll(torch.arange(b), 1).cuda()
    s, r = drive(su, su.x[:b][perm].contiguous(), tgt[perm].contiguous(), raw0[perm].contiguous(), mode, [N])
    for p, q in zip(s[0], base_s[0]):
        assert same(p, q[perm]), f"{su.label} {mode}: rows of a permuted batch are not the permuted rows"
    assert same(r, base_r[:, perm])
    if key == ("seq", "P3"):
        return
    for c in range(b):
        s, r = drive(su, su.x[c:c + 1], tgt[c:c + 1], raw0[c:c + 1], mode, [N])
        for p, q in zip(s[0], base_s[0]):
            assert same(p, q[c:c + 1]), f"{su.label} {mode}: clip {c} alone differs from its row in the batch of {b}"
        assert same(r, base_r[:, c:c + 1])


def test_plain_eps_does_not_reproduce_the_tf_driver():
    """ivf_tfclstm_search hands ivf_search_step eps_hat(step) = eps / sqrtf(1 - powf(beta2, step)); test_driver_equals_
    its_pieces replays it with that value.  The same replay with plain eps must leave the driver's bits within N
    steps: eps_hat(1) = 3.2e-7 against gradients of 1e-6 .. 1e-3 moves the first Adam step by 1e-4 .. 1e-1 of itself."""
    su = setup_of(("seq", "TF"))
    b = su.B
    res = both(su, "freeze", b)
    states, rows, _ = replay(su, su.x[:b], su.targets[:b].contiguous(), res["raw0"], "freeze", plain_eps=True)
    differs = [k + 1 for k in range(N) if not same(states[k][0], res["states"][k][0])]
    ulps = (bits(states[-1][0]).long() - bits(res["states"][-1][0]).long()).abs()
    note(f"search driver TF: the replay with plain eps leaves the driver's raw mask at iteration {differs[:1]}, after {N} "
         f"iterations {int((ulps > 0).sum())}/{ulps.numel()} entries differ, by up to {int(ulps.max())} ulp")
    assert differs and differs[0] <= N
    assert same(rows[0], res["rows"][0])          # the first trajectory row is written before eps is used


@pytest.mark.parametrize("key", [("i3d", "gray", "fp32"), ("seq", "S1"), ("seq", "TF")], ids=_id)
def test_a_regulariser_two_per_mille_off_is_seen(key):
    """the comparison can see what it is there for: the same replay with lam1 * 1.002 leaves the driver's bits.  Adam's
    first step is nearly blind to the size of the gradient (lr g / (|g| + eps)), so the first iteration shows in the
    trajectory row and in exp_avg, the raw mask from the second step on."""
    su = setup_of(key)
    b = su.sizes[-1]
    res = both(su, "freeze", b)
    states, rows, _ = replay(su, su.x[:b], su.targets[:b].contiguous(), res["raw0"], "freeze", lam1=R.LAM1 * 1.002)
    assert not same(rows[0], res["rows"][0]) and not same(states[0][1], res["states"][0][1])
    assert not same(states[-1][0], res["states"][-1][0])


# ---------------------------------------------------------------------------------------------------- 2. chain vs float64
@pytest.mark.parametrize("pid,mode", R.RUNS, ids=_id)
def test_chain_matches_float64_on_the_gpus_own_masks(pid, mode):
    """sig, probs, score and d score / d sig of the pieces at every iteration of the replay (which part 1 proves is the
    driver's) against search_refs.chain in float64 on the raw the GPU had, per clip (clstm_refs.elem_err), at
    GATE_MARGIN x the float32 floor of the same tensor on the same raw.  A clip with an ambiguous pool window at that
    iteration is left out of d score / d sig only: none in S1, S2 and TF, at most 1/16 of the clips in P3."""
    su = setup_of(("seq", pid))
    plan = R.PLANS[pid]
    b = plan.b
    res = both(su, mode, b)
    x, net, targets = R.inputs(pid)
    cap = R.ambiguous_cap(pid, b)
    failures = []
    for it, rec in enumerate(res["recs"]):
        ms = R.measure(pid, x[:b], net, targets[:b], rec["raw"].cpu(), mode)
        got = {"sig": rec["sig"], "probs": rec["probs"], "score": rec["score"].view(b, 1), "dsig": rec["dsig"]}
        left = [int(r) for r in np.nonzero(ms["ambiguous"])[0]]
        assert len(left) <= cap, f"{pid} {mode} iteration {it + 1}: clips {left} are ambiguous (cap {cap})"
        for name in R.TENSORS:
            e = CR.elem_err(got[name].cpu().numpy().astype(np.float64), ms["ref"][name])
            kept = [r for r in range(b) if not (name == "dsig" and r in left)]
            worst = float(np.max(e[kept]))
            fl, gate = ms["floor"][name], ms["gate"][name]
            note(f"search driver {pid} {mode} b={b}/B={su.B} iteration {it + 1} {name}: floor {fl:.3e} gpu {worst:.3e} "
                 f"ratio {worst / fl:.2f} (gate {CR.GATE_MARGIN:g}x, clips compared {len(kept)}/{b})")
            if not worst <= gate:
                failures.append(f"iteration {it + 1} {name}: {worst:.3e} > gate {gate:.3e}, clips {[r for r in kept if not e[r] <= gate][:8]}")
    assert not failures, "; ".join(failures)


# ---------------------------------------------------------------------------------------------------- 3. I3D input gradient
@pytest.mark.parametrize("key,mode", [(("i3d",) + p, m) for p in I3D_PLANS for m in R.MODES], ids=_id)
def test_i3d_input_gradient_through_the_mask_backward(key, mode):
    """b = 2 < B: at every iteration the pad channels of the staged clip are +0.0 (C = 1 and C = 3), input:grad read back
    through the endpoint is the buffer the mask backward read, d score / d sig meets freeze_bwd_ref's b_dmask (freeze) or
    sum_bound(sum |term|, C HW) against reverse_bwd_ref (reverse), entry 0 (freeze) and every entry that is not the
    first half of a pair (reverse) is exactly 0.0, and NaN in the pad channels of a copy of the gradient changes no bit
    of it.  After the driver's own first iteration input:grad holds the same bits."""
    su = setup_of(key)
    pc, b = su.pc, 2
    C, T, HW = pc.C, pc.T, pc.HW
    xc = su.x[:b].cpu().view(b, C, T, HW)
    x = su.x[:b]
    seen = []

    def observe(step, rec, din):
        staged = pc.inbuf[:b]
        assert bool((bits(staged[..., C:]) == 0).all()), "pad channels of the staged clip"
        g4 = pc.eng.endpoint("input:grad", b)                                          # [b,4,T,H,W], pad channels included
        assert same(g4.view(b, 4, T, HW), din.permute(0, 3, 1, 2)), "input:grad is not the buffer the pieces read"
        g = g4[:, :C].contiguous()
        sig, dsig = rec["sig"].cpu(), rec["dsig"]
        gc = g.cpu().view(b, C, T, HW)
        if mode == "freeze":
            ref = mask_refs.freeze_bwd_ref(xc, gc, sig)
            err = inside(dsig, ref["dmask"], ref["b_dmask"], f"{su.label} freeze iteration {step}")
            worst = float((err[:, 1:] / ref["b_dmask"][:, 1:]).max())
            assert bool((bits(dsig[:, 0]) == 0).all())
        else:
            ref = LR.reverse_bwd_ref(xc, gc, sig)
            _, sa, first = LR.reverse_bwd_terms(xc, gc, sig)
            bound = LR.sum_bound(sa, C * HW)
            err = inside(dsig, ref, bound, f"{su.label} reverse iteration {step}")
            assert bool(first.any()) and bool((dsig.cpu()[~first] == 0).all())
            worst = float((err[first] / bound[first]).max())
        poisoned = din.clone()
        poisoned[..., C:] = float("nan")
        assert same(pc.mask_bwd(x, rec["sig"], poisoned, b, mode), dsig), "the mask backward reads the pad channels"
        seen.append((g4, worst))

    res = both(su, mode, b, observe=observe)
    assert len(seen) == N
    assert same(res["din1"], seen[0][0]), "input:grad after the driver's first iteration differs from the pieces'"
    note(f"search driver {su.label} {mode} b={b}/B={su.B}: d score / d sig through the plan's input:grad, worst err/bound per "
         f"iteration {' '.join(f'{w:.2e}' for _, w in seen)}")


def test_wall_time_of_this_file():
    note(f"search driver: wall time of tests/test_gpu_search_driver.py {time.time() - _T0[0]:.0f} s")
