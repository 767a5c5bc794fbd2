"""CPU test of tests/ig_refs.py and of the host side of csrc/ig_ops.hip: the fp64 references against torch autograd and
the completeness axiom, every bound used on the GPU against an emulation of the kernels' own fp32 arithmetic, what wrong
implementations would do to the gates, the fixture's own noise floor, and the argument checks of the new entries -- on
the very inputs test_gpu_ig.py later runs the kernels on.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import clstm_refs as CR
import ig_refs as R
from conftest import GOLDEN, note

F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------- (a) the reference
def test_pipeline_is_complete_on_a_quadratic():
    """The midpoint rule integrates a linear gradient exactly: on f(p) = a.p + p.Q p the fp64 pipeline's total equals
    f(x) - f(x0) to rounding, and its gradient path equals torch autograd's, for each baseline kind"""
    g = np.random.default_rng(3)
    B, C, T, H, W = 2, 2, 3, 2, 3
    n = C * T * H * W
    a, Q = g.normal(size=n), g.normal(size=(n, n)) / n
    x = g.uniform(0, 1, (B, C, T, H, W))

    def f(p):
        p = p.reshape(len(p), -1)
        return p @ torch.from_numpy(a) + ((p @ torch.from_numpy(Q)) * p).sum(1)

    def grad_fn(pts):
        p = torch.from_numpy(pts).requires_grad_()
        s = f(p)
        s.sum().backward()
        return s.detach().numpy(), p.grad.numpy()

    for kind in R.KINDS.values():
        x0 = R.baseline(x, kind, base=g.uniform(0, 1, x.shape), value=0.25)
        alpha, w = R.midpoint(4)
        out = R.ig_pipeline(x, x0, alpha, w, grad_fn)
        want = f(torch.from_numpy(x)).numpy() - f(torch.from_numpy(x0)).numpy()
        assert np.max(np.abs(out["total"] - want)) <= 1e-12 * np.max(np.abs(want))
        assert np.allclose(out["frames"], out["map"].sum((2, 3)), rtol=1e-13, atol=0)
        if kind == R.FROZEN:
            assert np.all(out["map"][:, 0] == 0.0) and np.all(out["abs_frames"][:, 0] == 0.0)
        # left-Riemann is NOT exact here: the test can tell the rules apart
        al, wl = R.left_riemann(4)
        off = R.ig_pipeline(x, x0, al, wl, grad_fn)["total"]
        assert np.max(np.abs(off - want)) > 1e-3 * np.max(np.abs(want))


def test_midpoint_rule_values():
    a, w = R.midpoint(32)
    assert a.dtype == F32 and w.dtype == F32
    assert np.array_equal(a, ((2 * np.arange(32) + 1) / 64.0).astype(F32)) and np.all(w == F32(1 / 32))
    a, w = R.midpoint(3)
    assert abs(float(a.astype(F64).mean()) - 0.5) < 1e-7 and abs(float(w.astype(F64).sum()) - 1) < 1e-7


# ---------------------------------------------------------------------------------------------------- (b) stage bound
def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 numbers is exact in float64; the float64 sum then rounds to fp32.
    (Double rounding can move the last bit in rare cases; the bounds below have room for it, nothing bit-exact rests
    on it.)"""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


@pytest.mark.parametrize("kind", list(R.KINDS.values()), ids=list(R.KINDS))
def test_stage_bound_holds_for_the_kernel_arithmetic(kind):
    worst = 0.0
    for shape in R.STAGE_SHAPES[::7]:
        x, base, value = R.stage_inputs(shape, kind)
        x0 = R.baseline(x, kind, base, value)
        alpha = R.kernel_alpha(shape[4])
        assert np.all((alpha >= 0) & (alpha <= 1))
        ref, bound = R.stage_ref(x, x0, alpha), R.stage_bound(x, x0)
        d = (x - x0).astype(F32)
        got = np.stack([_fma32(np.full_like(d, a), d, x0) for a in alpha], 1)
        err = np.abs(got.astype(F64) - ref)
        assert np.all(err <= bound)
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        same = (x == x0)
        assert same.mean() > 0.1                                   # the exact case is populated
        assert np.array_equal(got[np.broadcast_to(same[:, None], got.shape)],
                              np.broadcast_to(x0[:, None], got.shape)[np.broadcast_to(same[:, None], got.shape)])
        for k in np.nonzero(alpha == 0)[0]:
            assert np.array_equal(got[:, k], x0)
        # the unfused expression (product rounded, then the sum) is NOT within the bound everywhere it could be:
        # its worst case is 5 U m, so the kernel must fuse
    note(f"ig stage kind {kind}: fp32 emulation uses {worst:.2f} of the gamma(3) bound")
    assert worst > 0.05          # the bound is not vacuous


def test_windows_cover_the_required_geometry():
    for B, K in ((1, 1), (1, 8), (3, 1), (3, 3), (3, 8)):
        ws = R.windows(B, K)
        assert ws[0] == (0, B * K)
        for first, count in ws:
            assert 0 <= first and count >= 1 and first + count <= B * K
        if B == 3:      # some window crosses two clip boundaries and (K > 1) starts mid-clip
            assert any({(first + j) // K for j in range(count)} == {0, 1, 2} and (K == 1 or first % K != 0)
                       for first, count in ws)


# ---------------------------------------------------------------------------------------------------- (c) accumulate, finish
@pytest.mark.parametrize("shape", R.ACC_SHAPES, ids=[str(s) for s in R.ACC_SHAPES])
def test_accumulate_and_finish_bounds_hold_for_fp32(shape):
    din, w = R.acc_inputs(shape)
    ref, bound = R.gsum_ref(din, w)
    got = R.gsum_fp32(din, w)
    assert np.all(np.abs(got.astype(F64) - ref) <= bound)
    B, C, T, HW, K = shape
    for kind in R.KINDS.values():
        x, base, value, gsum = R.finish_inputs(shape, kind)
        x0 = R.baseline(x, kind, base, value)
        f = R.finish_ref(x, x0, gsum)
        A = ((x - x0).astype(F32) * gsum).astype(F32)
        m = np.zeros((B, T, HW), F32)
        for c in range(C):
            m = (m + A[:, c]).astype(F32)
        assert np.all(np.abs(m.astype(F64) - f["map"]) <= f["b_map"])
        fr = np.zeros((B, T), F32)
        for px in range(HW):                                      # one fixed order of many
            fr = (fr + m[:, :, px]).astype(F32)
        assert np.all(np.abs(fr.astype(F64) - f["frames"]) <= f["b_frames"])
        tot = np.zeros(B, F32)
        for t in range(T):
            tot = (tot + fr[:, t]).astype(F32)
        assert np.all(np.abs(tot.astype(F64) - f["total"]) <= f["b_total"])
        if kind == R.FROZEN:
            assert np.all(m[:, 0] == 0.0) and np.all(f["abs_frames"][:, 0] == 0.0)


def test_kernel_mutants_leave_the_bounds():
    """a gradient row read from the wrong node, a weight of the wrong node, a pad lane read as a channel: each is far
    outside the accumulate bound on these inputs"""
    shape = R.ACC_SHAPES[2]
    din, w = R.acc_inputs(shape)
    ref, bound = R.gsum_ref(din, w)
    for wrong in (R.gsum_fp32(din[:, ::-1], w), R.gsum_fp32(din, np.roll(w, 1)), R.gsum_fp32(np.roll(din, 1, axis=2), w)):
        assert np.mean(np.abs(wrong.astype(F64) - ref) > 100 * bound) > 0.5


# ---------------------------------------------------------------------------------------------------- (d) the chain case
@pytest.mark.parametrize("name", [b[0] for b in R.CHAIN_BASELINES])
def test_chain_has_no_ambiguous_window_on_any_path_row(name):
    b = R.chain_reference(name)
    assert b["ambiguous"].shape == (len(R.CHAIN_IDS) * R.CHAIN_K,)
    assert int(b["ambiguous"].sum()) == 0, b["ambiguous"]
    for n in R.CHAIN_TENSORS:
        note(f"ig chain {name} {n}: float32 floor {b['floor'][n]:.3e}, gate {b['gate'][n]:.3e}")
    gap = b["ref"]["total"] - 0.0
    note(f"ig chain {name}: reference ig_total {gap}, path scores {b['ref']['path_scores'].tolist()}")
    if name == "frozen":
        assert np.all(b["ref"]["map"][:, 0] == 0.0)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_chain_mutants_land_many_gates_away(mutant):
    for name, _, _ in R.CHAIN_BASELINES:
        if mutant == "prevframe" and name != "frozen":
            continue
        b = R.chain_reference(name)
        out = R.chain_mutant(b, mutant)
        ratios = {n: float(np.min(R.chain_err(out[n], b["ref"][n]))) / b["gate"][n] for n in ("map", "frames")}
        note(f"ig chain {name} mutant {mutant}: " + ", ".join(f"{n} {v:.1f} gates" for n, v in ratios.items()))
        assert ratios["map"] > 100, (name, mutant, ratios)          # every clip, the map
        assert ratios["frames"] > 100, (name, mutant, ratios)


# ---------------------------------------------------------------------------------------------------- (e) the I3D fixture
def test_fixture_noise_floor_is_inside_half_the_gate():
    """The fixture's fp64 and 4-thread runs against its fp32 / 8-thread run: sampled map and abs_frames inside half the
    whole-chain gates; frames and total (cancellation figures) inside half the gate times abs_frames.  Black baseline:
    the reference's own |ig_gap| is below 1 % of score_x - score_base at K = 8."""
    g = dict(np.load(os.path.join(GOLDEN, "ig.npz")))
    assert int(g["K"]) == 8 and tuple(g["clips"]) == R.I3D_CLIPS
    l2_gate, max_gate = R.I3D_L2_GATE[True], R.I3D_MAX_GATE[True]
    for cid in R.I3D_CLIPS:
        for tag, _, _ in R.I3D_BASELINES:
            p = f"c{cid}_{tag}"
            ref, af = g[f"{p}_map_val"], g[f"{p}_abs_frames"]
            assert np.all(af[1:] > 0)
            if tag == "frozen":
                assert af[0] == 0.0 and g[f"{p}_frames"][0] == 0.0
            for leg in ("f64", "f32t4"):
                q = f"{leg}_{p}"
                l2 = np.linalg.norm(g[f"{q}_map_val"] - ref) / np.linalg.norm(ref)
                mx = np.max(np.abs(g[f"{q}_map_val"] - ref)) / np.max(np.abs(ref))
                ea = np.max(np.abs(g[f"{q}_abs_frames"] - af)[af > 0] / af[af > 0])
                ef = np.max(np.abs(g[f"{q}_frames"] - g[f"{p}_frames"])[af > 0] / af[af > 0])
                et = abs(float(g[f"{q}_total"]) - float(g[f"{p}_total"])) / af.sum()
                note(f"ig fixture {p} {leg}: map L2 {l2:.2e} max {mx:.2e}, abs_frames {ea:.2e}, frames/abs_frames "
                     f"{ef:.2e}, total/sum abs_frames {et:.2e}")
                assert l2 <= 0.5 * l2_gate and mx <= 0.5 * max_gate and ea <= 0.5 * l2_gate
                assert ef <= 0.5 * l2_gate and et <= 0.5 * l2_gate
            if tag == "black":
                drop = float(g[f"{p}_score_x"]) - float(g[f"{p}_score_base"])
                gap = float(g[f"{p}_total"]) - drop
                note(f"ig fixture {p}: total {float(g[f'{p}_total']):.6f}, f(x) - f(x0) {drop:.6f}, gap {gap:.2e}")
                assert abs(gap) < 1e-2 * abs(drop)


# ---------------------------------------------------------------------------------------------------- (f) argument checks
def test_bad_arguments_return_error_codes():
    import ivf_lib as L
    lib = L.lib()
    one = ctypes.c_void_p(256)          # a non-null address that is never dereferenced: every call below is refused
    assert lib.ivf_ig_stage(None, 0, None, 0.0, None, 1, 3, 4, 10, 2, 0, 1, None, 0, None) == -1
    assert b"ig_stage" in lib.ivf_last_error()
    assert lib.ivf_ig_stage(one, 3, None, 0.0, one, 1, 3, 4, 10, 2, 0, 1, one, 0, None) == -1      # kind
    assert lib.ivf_ig_stage(one, 2, None, 0.0, one, 1, 3, 4, 10, 2, 0, 1, one, 0, None) == -1      # 'clip' without base
    assert lib.ivf_ig_stage(one, 0, None, 0.0, one, 1, 3, 4, 10, 2, 1, 2, one, 0, None) == -1      # rows past b*K
    assert lib.ivf_ig_stage(one, 0, None, 0.0, one, 1, 5, 4, 10, 2, 0, 1, one, 4, None) == -1      # C > 4 channels-last
    assert lib.ivf_ig_stage(one, 0, None, 0.0, one, 1, 3, 4, 10, 2, 0, 1, one, 8, None) == -1      # layout
    assert lib.ivf_ig_accumulate(None, 0, None, 2, 0, 1, None, 1, 3, 4, 10, None) == -1
    assert lib.ivf_ig_accumulate(one, 0, one, 2, 2, 1, one, 1, 3, 4, 10, None) == -1               # rows past b*K
    assert lib.ivf_ig_finish(None, 0, None, 0.0, None, 1, 3, 4, 10, None, None, None, None, None) == -1
    assert lib.ivf_ig_workspace_bytes(0, 3, 4, 10, 2) == 0
    # Gsum + per-row targets + row scores, each 256-byte aligned
    assert lib.ivf_ig_workspace_bytes(2, 3, 16, 224 * 224, 32) == 2 * 3 * 16 * 224 * 224 * 4 + 256 + 256
    assert lib.ivf_ig_workspace_bytes(1, 1, 1, 1, 1) == 3 * 256
    for pfx in ("i3d", "clstm"):
        assert getattr(lib, f"ivf_{pfx}_ig")(None, None, 1, None, 0, None, 0.0, None, None, 4, *([None] * 7)) != 0
        assert getattr(lib, f"ivf_{pfx}_ig_path_scores")(None, None, 1, None, 0, None, 0.0, None, 4, None, None) != 0
    assert not hasattr(lib, "ivf_tfclstm_ig")
