"""SmoothGrad / SmoothGrad^2 / VarGrad (csrc/smoothgrad_ops.hip) on the GPU: the kernels against the fp64
references and bounds of tests/sg_refs.py (test_sg_refs_host.py proves those on the CPU, on the same inputs), the plain
gradient map against the plan's own backward, the whole method through the ConvLSTM plan against torch fp64 autograd, the
driver against its pieces, the I3D plan against the fixture tests/golden/smoothgrad.npz (torch autograd on the
reference's own model), and the Python surfaces.  Figures are written with note() before anything is asserted."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

import clstm_refs as CR
import ig_refs as IGR
import sg_refs as R
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


def _host(res):
    return {k: v.detach().cpu().numpy() for k, v in res.items()}


# ---------------------------------------------------------------------------------------------------- noise
@pytest.mark.parametrize("dims", [(1, 1, 35), (3, 5, 385)], ids=["35", "385x3x5"])
def test_noise_matches_fp64(dims):
    """ivf_sg_noise at k in {0, 1, 7} against the fp64 restatement: every element within Z_GATE_C U |z| (sg_refs derives
    the constant); the worst measured ratio is recorded (profiles/smoothgrad_parity.txt)"""
    L, lib = _lib()
    C, T, HW = dims
    worst = 0.0
    for seed in (0, R.SEED):
        for k in (0, 1, 7):
            z = torch.full((C * T * HW + 2,), float("nan"), device="cuda")
            L.check(lib.ivf_sg_noise(seed, k, 1, C, T, HW, ctypes.c_void_p(z.data_ptr() + 4), L.stream()))
            h = z.cpu().numpy()
            assert np.isnan(h[0]) and np.isnan(h[-1])
            got = h[1:-1].reshape(C, T, HW).astype(F64)
            ref = R.noise(seed, [k], C, T, HW)[0]
            err = np.abs(got - ref)
            nz = ref != 0
            ratio = float(np.max(err[nz] / (U * np.abs(ref[nz]))))
            worst = max(worst, ratio)
            note(f"sg noise {dims} seed {seed} k {k}: worst |z_gpu - z64| = {ratio:.2f} U |z| (gate {R.Z_GATE_C})")
            assert np.all(err <= R.z_gate(ref)), (dims, seed, k, ratio)
    note(f"sg noise {dims}: worst ratio {worst:.2f} U |z| of the gate's {R.Z_GATE_C}")
    # several samples in one call are the single-sample calls
    z = torch.empty(3, C, T, HW, device="cuda")
    L.check(lib.ivf_sg_noise(R.SEED, 5, 3, C, T, HW, L.ptr(z), L.stream()))
    one = torch.empty(C, T, HW, device="cuda")
    L.check(lib.ivf_sg_noise(R.SEED, 7, 1, C, T, HW, L.ptr(one), L.stream()))
    assert _same_bits(z[2].cpu().numpy(), one.cpu().numpy())


# ---------------------------------------------------------------------------------------------------- range
def test_range_is_exact():
    L, lib = _lib()
    for per_clip in R.RANGE_SIZES:
        x = R.range_inputs(per_clip)
        for level in (0.0, 0.15, 1.0):
            s = torch.full((len(x) + 2,), float("nan"), device="cuda")
            xd = _dev(x)
            L.check(lib.ivf_sg_range(L.ptr(xd), len(x), 1, 1, per_clip, level, ctypes.c_void_p(s.data_ptr() + 4), L.stream()))
            h = s.cpu().numpy()
            assert np.isnan(h[0]) and np.isnan(h[-1])
            assert _same_bits(h[1:-1], R.sigma_ref(x, level)), (per_clip, level)
        # an unaligned clip base takes the per-element kernel: the same bits
        buf = torch.zeros(len(x) * per_clip + 1, device="cuda")
        buf[1:] = _dev(x).reshape(-1)
        s = torch.empty(len(x), device="cuda")
        L.check(lib.ivf_sg_range(ctypes.c_void_p(buf.data_ptr() + 4), len(x), 1, 1, per_clip, 0.15, L.ptr(s), L.stream()))
        assert _same_bits(s.cpu().numpy(), R.sigma_ref(x, 0.15)), per_clip


# ---------------------------------------------------------------------------------------------------- stage
@pytest.mark.parametrize("layout", R.LAYOUTS, ids=["ncthw", "cl4"])
def test_stage_matches_fp64(layout):
    """Every shape of the table, every window: each element within U |p| + sigma (z gate) of fp64, equal to x bit for bit
    at level 0, pad lanes +0.0, nothing written outside the window's rows"""
    L, lib = _lib()
    worst, runs = 0.0, 0
    for shape in R.STAGE_SHAPES:
        B, C, T, HW, n = shape
        x = R.stage_inputs(shape)
        sigma = R.sigma_ref(x, R.LEVEL)
        ref, bound = R.stage_ref(x, sigma, R.noise(R.SEED, range(n), C, T, HW))
        ref, bound = ref.reshape(B * n, C, T, HW), bound.reshape(B * n, C, T, HW)
        xrows = np.broadcast_to(x[:, None], (B, n, C, T, HW)).reshape(B * n, C, T, HW)
        xd, sd, zero = _dev(x), _dev(sigma), torch.zeros(B, device="cuda")
        row = C * T * HW if layout == 0 else T * HW * 4
        for first, count in R.windows(B, n):
            for sg, want, bnd in ((sd, ref, bound), (zero, xrows, None)):
                buf = torch.full(((count + 2) * row,), float("nan"), device="cuda")
                out = ctypes.c_void_p(buf.data_ptr() + row * 4)
                L.check(lib.ivf_sg_stage(L.ptr(xd), L.ptr(sg), B, C, T, HW, n, R.SEED, first, count, out, layout, L.stream()))
                h = buf.cpu().numpy()
                assert np.isnan(h[:row]).all() and np.isnan(h[-row:]).all(), (shape, first, count)
                body = h[row:-row].reshape((count, C, T, HW) if layout == 0 else (count, T, HW, 4))
                rows, pads = R.from_layout(body, layout, C)
                if pads is not None:
                    assert not _bits(pads).any(), (shape, first, count)          # +0.0, bit for bit
                sl = slice(first, first + count)
                if bnd is None:
                    assert _same_bits(rows, want[sl]), (shape, first, count)      # level 0: x itself
                    continue
                err = np.abs(rows.astype(F64) - want[sl])
                assert not np.isnan(rows).any() and np.all(err <= bnd[sl]), (shape, first, count)
                worst = max(worst, float(np.max(err / bnd[sl])))
                runs += 1
    note(f"sg stage layout {layout}: {runs} windows, worst {worst:.2f} of the U |p| + sigma (z gate) bound")


def test_staged_noise_is_the_same_for_every_clip_and_layout():
    """with x = 0 and sigma = 1 the staged row IS z: row (clip, k) equals ivf_sg_noise's sample k bit for bit, for every
    clip, both layouts, the 16-byte and the per-element NCTHW kernel"""
    L, lib = _lib()
    for C, T, HW, n in ((3, 5, 385, 3), (2, 17, 388, 3), (1, 1, 35, 8)):
        B = 3
        z = torch.empty(n, C, T, HW, device="cuda")
        L.check(lib.ivf_sg_noise(R.SEED, 0, n, C, T, HW, L.ptr(z), L.stream()))
        zh = z.cpu().numpy()
        x, one = torch.zeros(B, C, T, HW, device="cuda"), torch.ones(B, device="cuda")
        for layout in R.LAYOUTS:
            out = torch.full((B * n,) + ((C, T, HW) if layout == 0 else (T, HW, 4)), float("nan"), device="cuda")
            L.check(lib.ivf_sg_stage(L.ptr(x), L.ptr(one), B, C, T, HW, n, R.SEED, 0, B * n, L.ptr(out), layout, L.stream()))
            rows, _ = R.from_layout(out.cpu().numpy(), layout, C)
            for b in range(B):
                assert _same_bits(rows[b * n:(b + 1) * n], zh), (C, T, HW, layout, b)


# ---------------------------------------------------------------------------------------------------- accumulate, finish
def _accumulate(L, lib, rows, n, wins, b, layout):
    """(G1, G2) [b,C,T,HW] after the windows `wins` of the row list `rows` [b*n,C,T,HW]; din has NaN pad lanes"""
    _, C, T, HW = rows.shape
    G1, G2 = torch.zeros(b, C, T, HW, device="cuda"), torch.zeros(b, C, T, HW, device="cuda")
    for first, count in wins:
        din = _dev(R.to_layout(rows[first:first + count], layout, pad=np.nan))
        L.check(lib.ivf_sg_accumulate(L.ptr(din), layout, n, first, count, L.ptr(G1), L.ptr(G2), b, C, T, HW, L.stream()))
    return G1.cpu().numpy(), G2.cpu().numpy()


def _finish(L, lib, G1, G2, n):
    B, C, T, HW = G1.shape
    maps = [torch.full((B, T, HW), float("nan"), device="cuda") for _ in range(3)]
    frames = [torch.full((B, T), float("nan"), device="cuda") for _ in range(3)]
    g1, g2 = _dev(G1), _dev(G2)
    L.check(lib.ivf_sg_finish(L.ptr(g1), L.ptr(g2), n, B, C, T, HW, *[L.ptr(t) for t in maps + frames], L.stream()))
    names = ("sg", "sq", "var", "sg_frames", "sq_frames", "var_frames")
    return {k: t.cpu().numpy() for k, t in zip(names, maps + frames)}


@pytest.mark.parametrize("layout", R.LAYOUTS, ids=["ncthw", "cl4"])
def test_accumulate_matches_fp64_and_is_window_invariant(layout):
    L, lib = _lib()
    for shape in R.ACC_SHAPES:
        B, C, T, HW, n = shape
        din = R.acc_inputs(shape)
        rows = din.reshape(B * n, C, T, HW)
        N = B * n
        g1, g2 = _accumulate(L, lib, rows, n, [(0, N)], B, layout)
        r1, r2, b1, b2 = R.moments_ref(din)
        e1, e2 = np.abs(g1.astype(F64) - r1), np.abs(g2.astype(F64) - r2)
        note(f"sg accumulate {shape} layout {layout}: G1 worst {float(np.max(e1 / np.maximum(b1, 1e-300))):.2f} of "
             f"gamma(n) sum|g|, G2 worst {float(np.max(e2 / b2)):.2f} of gamma(n+1) sum g^2")
        assert not np.isnan(g1).any() and not np.isnan(g2).any() and np.all(e1 <= b1) and np.all(e2 <= b2), shape
        splits = []
        if N >= 2:
            splits.append([(0, N // 2), (N // 2, N - N // 2)])
        if N >= 3:
            splits.append([(0, 1), (1, N - 2), (N - 1, 1)])              # cuts inside clips, a window over several
        for wins in splits:
            w1, w2 = _accumulate(L, lib, rows, n, wins, B, layout)
            assert _same_bits(w1, g1) and _same_bits(w2, g2), (shape, wins)
        for r in range(B):                                              # batched rows == one-clip calls
            s1, s2 = _accumulate(L, lib, din[r], n, [(0, n)], 1, layout)
            assert _same_bits(s1[0], g1[r]) and _same_bits(s2[0], g2[r]), (shape, r)


def test_finish_matches_fp64():
    L, lib = _lib()
    for shape in R.ACC_SHAPES:
        B, C, T, HW, n = shape
        a1, a2 = R.moments_fp32(R.acc_inputs(shape))
        f, got = R.finish_ref(a1, a2, n), _finish(L, lib, a1, a2, n)
        figs = []
        for k in ("sg", "sq", "var", "sg_frames", "sq_frames", "var_frames"):
            err = np.abs(got[k].astype(F64) - f[k])
            figs.append(f"{k} {float(np.max(err / np.maximum(f[f'b_{k}'], 1e-300))):.3f}")
            assert not np.isnan(got[k]).any() and np.all(err <= f[f"b_{k}"]), (shape, k)
        note(f"sg finish {shape}: share of the bound used: " + ", ".join(figs))
        if n == 1:
            assert not _bits(got["var"]).any() and not _bits(got["var_frames"]).any()      # exactly +0.0
        for r in range(B):
            solo = _finish(L, lib, a1[r:r + 1], a2[r:r + 1], n)
            for k in got:
                assert _same_bits(solo[k][0], got[k][r]), (shape, r, k)


# ---------------------------------------------------------------------------------------------------- plain gradient
def _clstm_engine(case, max_batch, sd):
    import ivf_engine
    eng = ivf_engine.CLSTMEngine(CR.K, (case.C, case.T, case.H, case.W), max_batch=max_batch, hidden=case.hid,
                                 layers=case.layers, kernel=case.k, stride=case.s, softmax=case.softmax,
                                 batch_norm=case.batch_norm)
    eng.load_state_dict(sd)
    return eng


def _abs_channel_sum(dx):
    """|dx_0| + |dx_1| + ... in fp32, in that order, from +0.0"""
    m = torch.zeros_like(dx[:, 0])
    for c in range(dx.shape[1]):
        m = m + dx[:, c].abs()
    return m.cpu().numpy()


def test_plain_gradient_is_the_plans_backward_clstm():
    """smoothgrad(n_samples=1, level=0)['sg_map'] == sum_c |dx_c| of engine.backward, bit for bit; sq_map == sum_c dx_c^2"""
    case, x, sd, targets = R.chain_inputs()
    eng = _clstm_engine(case, case.B, sd)
    xd = _dev(x)
    got = _host(eng.smoothgrad(xd, targets, n_samples=1, level=0.0))
    eng.forward(xd)
    score, dx = eng.backward(len(x), target=targets)
    assert _same_bits(got["sg_map"], _abs_channel_sum(dx))
    assert _same_bits(got["sample_scores"][:, 0], score.cpu().numpy())
    assert not _bits(got["var_map"]).any() and not _bits(got["sigma"]).any()
    sq = torch.zeros_like(dx[:, 0])
    for c in range(dx.shape[1]):
        sq = sq + dx[:, c] * dx[:, c]
    assert _same_bits(got["sq_map"], sq.cpu().numpy())


def test_plain_gradient_is_the_plans_backward_i3d():
    import ivf_engine
    import ivf_recipe as RC
    eng = ivf_engine.I3DEngine(174, (3, 16, 224, 224), max_batch=1, softmax=True)
    eng.load_state_dict(RC.i3d_state_dict(num_classes=174))
    x = torch.from_numpy(RC.clip(21))[None].cuda()
    target = [int(eng.argmax(eng.forward(x))[0])]
    got = _host(eng.smoothgrad(x, target, n_samples=1, level=0.0))
    eng.forward(x)
    _, dx = eng.backward(1, target=target)
    want = _abs_channel_sum(dx)
    note(f"sg plain gradient i3d: max |sg_map - sum_c |dx_c|| = {float(np.max(np.abs(got['sg_map'] - want))):.3e} "
         f"of max {float(want.max()):.3e}")
    assert _same_bits(got["sg_map"], want)


# ---------------------------------------------------------------------------------------------------- the ConvLSTM chain
_KEYS = {"sg": "sg_map", "sq": "sq_map", "var": "var_map", "sg_frames": "sg_frames", "sq_frames": "sq_frames",
         "var_frames": "var_frames", "sample_scores": "sample_scores"}


@pytest.mark.parametrize("level", R.CHAIN_LEVELS)
def test_chain_matches_fp64_autograd(level):
    """Case S2, n = 4: the three maps, their frame sums and the sample scores of every clip against torch fp64 autograd
    through clstm_refs' functional model on noisy inputs built from the fp64 z, at GATE_MARGIN x the float32 floor of the
    same tensor"""
    b = R.chain_reference(level)
    assert int(b["ambiguous"].sum()) == 0                     # no clip is left out (test_sg_refs_host.py)
    case, x = b["case"], _dev(b["x"])
    eng = _clstm_engine(case, case.B, b["sd"])
    got = _host(eng.smoothgrad(x, b["targets"], n_samples=R.CHAIN_N, level=level, seed=R.CHAIN_SEED))
    ref = b["ref"]
    assert _same_bits(got["sigma"], R.sigma_ref(b["x"], level))
    worst = {n: float(np.max(IGR.chain_err(got[_KEYS[n]].reshape(ref[n].shape), ref[n]))) for n in R.TENSORS}
    for n, v in worst.items():
        note(f"sg chain level {level} {n}: floor {b['floor'][n]:.3e} gpu {v:.3e} ratio {v / b['floor'][n]:.2f} "
             f"(gate {CR.GATE_MARGIN:g}x)")
    for n, v in worst.items():
        assert v <= b["gate"][n], (level, n, v, b["gate"][n])


def test_driver_equals_its_pieces_and_one_clip_calls():
    """ivf_clstm_smoothgrad on a plan of 3 rows, b = 2, n = 4 (chunks of 3 rows cross the clip boundary) equals the kernels
    called one by one around the plan's forward and backward, and equals one-clip calls, bit for bit"""
    L, lib = _lib()
    case, x, sd, targets = R.chain_inputs()
    eng = _clstm_engine(case, 3, sd)
    n, b = R.CHAIN_N, x.shape[0]
    C, T, H, W = eng.clip_shape
    HW = H * W
    xd = _dev(x)
    for level in R.CHAIN_LEVELS:
        whole = _host(eng.smoothgrad(xd, targets, n_samples=n, level=level, seed=R.CHAIN_SEED))
        sigma = torch.empty(b, device="cuda")
        L.check(lib.ivf_sg_range(L.ptr(xd), b, C, T, HW, level, L.ptr(sigma), L.stream()))
        G1, G2 = torch.zeros(b, C, T, HW, device="cuda"), torch.zeros(b, C, T, HW, device="cuda")
        scores = torch.empty(b * n, device="cuda")
        rowt = [t for t in targets for _ in range(n)]
        for first in range(0, b * n, eng.max_batch):
            cnt = min(eng.max_batch, b * n - first)
            p = torch.empty(cnt, C, T, H, W, device="cuda")
            L.check(lib.ivf_sg_stage(L.ptr(xd), L.ptr(sigma), b, C, T, HW, n, R.CHAIN_SEED, first, cnt, L.ptr(p), 0, L.stream()))
            eng.forward(p)
            sc, dx = eng.backward(cnt, target=rowt[first:first + cnt])
            scores[first:first + cnt] = sc
            L.check(lib.ivf_sg_accumulate(L.ptr(dx), 0, n, first, cnt, L.ptr(G1), L.ptr(G2), b, C, T, HW, L.stream()))
        parts = _finish(L, lib, G1.cpu().numpy(), G2.cpu().numpy(), n)
        for k in ("sg", "sq", "var"):
            assert _same_bits(whole[f"{k}_map"].reshape(b, T, HW), parts[k]), (level, k)
            assert _same_bits(whole[f"{k}_frames"], parts[f"{k}_frames"]), (level, k)
        assert _same_bits(whole["sample_scores"], scores.cpu().numpy().reshape(b, n))
        assert _same_bits(whole["sigma"], sigma.cpu().numpy())
        for r in range(b):
            solo = _host(eng.smoothgrad(xd[r:r + 1], targets[r:r + 1], n_samples=n, level=level, seed=R.CHAIN_SEED))
            for key in whole:
                assert _same_bits(solo[key][0], whole[key][r]), (level, r, key)
    other = _host(eng.smoothgrad(xd, targets, n_samples=n, level=0.15, seed=R.CHAIN_SEED + 1))
    assert not _same_bits(other["sg_map"], whole["sg_map"])            # the seed matters
    for bad in (dict(n_samples=0), dict(level=-0.1), dict(level=float("nan")), dict(seed=-1), dict(seed=2 ** 32)):
        with pytest.raises(L.IvfError):
            eng.smoothgrad(xd, targets, **bad)
    zs = eng.sg_noise(2, seed=R.CHAIN_SEED, first=1).cpu().numpy()
    assert zs.shape == (2, C, T, H, W)
    assert np.all(np.abs(zs.reshape(2, C, T, HW) - R.noise(R.CHAIN_SEED, [1, 2], C, T, HW)) <= R.z_gate(
        R.noise(R.CHAIN_SEED, [1, 2], C, T, HW)))


# ---------------------------------------------------------------------------------------------------- I3D against the fixture
@pytest.mark.parametrize("math", ["fp32", "bf16x3", "bf16x6"])
def test_i3d_matches_fixture(math, golden):
    """Clips 21 and 7 in one call on a plan of 3 rows, n = 8, level 0.15: sampled sg_map and sq_map at the whole-chain
    d(score)/d(input) gates of test_gpu_i3d.py, their frames at that gate times the frame's magnitude sum (the terms are
    non-negative: the sum itself), sample scores at 1e-3; var_map against the fixture's own spread between its fp32, fp64
    and 4-thread legs times LEG_FACTOR (sg_refs.i3d_var_gates), var_frames at the whole-chain gate times sq_frames.
    The legs are fp32-class runs, so their spread is a gate for the fp32-class arithmetic modes (fp32, bf16x6) only.
    The 3-pass split bf16x3 is not fp32-class -- test_gpu_i3d.py gives it whole-chain gates of its own -- and its
    var_map is held at those, like its sg_map and sq_map: with sum var (n - 1) / sum G2 = 0.87 on this fixture var_map
    cancels little and inherits the error of sq_map.

    Measured on the MI355X (DESIGN 15 has the table), worst over the clips, map L2 / max: fp32 sg 4.5e-3 / 1.2e-2, sq
    2.9e-3 / 8.7e-3, var 3.1e-3 / 1.1e-2; bf16x6 sg 5.9e-3 / 1.4e-2, sq 3.6e-3 / 1.1e-2, var 3.9e-3 / 1.3e-2 against var
    gates of 5.5e-3 / 1.4e-2 (clip 21) and 6.2e-3 / 2.2e-2 (clip 7); bf16x3 sg 1.6e-2 / 3.0e-2, sq 1.1e-2 / 1.6e-2, var
    1.1e-2 / 2.2e-2 -- three times bf16x6 on all three maps alike, which is the arithmetic mode and not the variance
    formula, and outside the fp32-class spread.  The figures are written by note() on every run."""
    import ivf_engine
    import ivf_recipe as RC
    g = golden("smoothgrad")
    n = int(g["n"])
    exact = math in R.I3D_EXACT
    l2_gate, max_gate = R.I3D_L2_GATE[exact], R.I3D_MAX_GATE[exact]
    eng = ivf_engine.I3DEngine(174, (3, 16, 224, 224), max_batch=3, softmax=True, math=math)
    eng.load_state_dict(RC.i3d_state_dict(num_classes=174))
    x = torch.from_numpy(np.stack([RC.clip(c) for c in R.I3D_CLIPS])).cuda()
    targets = [int(g[f"c{c}_target"]) for c in R.I3D_CLIPS]
    got = _host(eng.smoothgrad(x, targets, n_samples=n, level=float(g["level"]), seed=int(g["seed"])))
    fails = []
    for i, cid in enumerate(R.I3D_CLIPS):
        p = f"c{cid}"
        idx = g[f"{p}_idx"]
        assert _same_bits(got["sigma"][i], g[f"{p}_sigma"])
        checks = {}
        for k in ("sg", "sq", "var"):
            ref = g[f"{p}_{k}_val"].astype(F64)
            sample = got[f"{k}_map"][i].ravel()[idx].astype(F64)
            l2, mx = np.linalg.norm(sample - ref) / np.linalg.norm(ref), rel_err(sample, ref)
            mag = g[f"{p}_sq_frames"] if k == "var" else g[f"{p}_{k}_frames"]
            ef = float(np.max(np.abs(got[f"{k}_frames"][i] - g[f"{p}_{k}_frames"]) / mag))
            gl2, gmx = R.i3d_var_gates(g, cid) if k == "var" and exact else (l2_gate, max_gate)
            note(f"sg i3d {math} {p} {k}: map L2 {l2:.2e} max {mx:.2e} (gates {gl2:.3g} {gmx:.3g}); frames {ef:.2e} "
                 f"(gate {l2_gate:g})")
            checks.update({f"{k} L2": l2 < gl2, f"{k} max": mx < gmx, f"{k} frames": ef < l2_gate})
        es = rel_err(got["sample_scores"][i], g[f"{p}_sample_scores"])
        canc = float(got["var_frames"][i].astype(F64).sum() * (n - 1) / (got["sq_frames"][i].astype(F64).sum() * n))
        note(f"sg i3d {math} {p}: sample scores {es:.2e}; sum var (n - 1) / sum G2 gpu {canc:.4f} ref "
             f"{float(g[f'{p}_cancellation']):.4f}")
        checks["sample scores"] = es < 1e-3
        checks["score_x"] = abs(float(got["score_x"][i]) - float(g[f"{p}_score_x"])) < 1e-3 * float(g[f"{p}_score_x"])
        fails += [(p, name) for name, ok in checks.items() if not ok]
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


def test_smoothgrad_video_i3d(smth_model):
    import ivf_lib as L
    import ivf_recipe as RC
    from smoothgrad_videos import SmoothGradVideo
    x = torch.from_numpy(RC.clip(21))[None]
    sgv = SmoothGradVideo(smth_model, n_samples=2, level=0.1, seed=3)
    m, out = sgv(x)
    assert m.shape == (16, 224, 224) and m.dtype == np.float32 and tuple(out.shape) == (1, 174)
    assert np.isfinite(m).all() and (m >= 0).all() and m.any()
    assert _same_bits(m, sgv.last["sg_map"][0].cpu().numpy())
    mv, _ = SmoothGradVideo(smth_model, n_samples=2, level=0.1, seed=3, kind="var")(x, index=int(torch.argmax(out[0])))
    assert _same_bits(mv, sgv.last["var_map"][0].cpu().numpy()) and not _same_bits(mv, m)
    fr = sgv.last["sg_frames"][0].cpu().numpy()
    assert np.all(np.abs(fr - m.astype(F64).sum((1, 2))) <= sum_bound(np.abs(m).sum((1, 2)), 224 * 224) + U * np.abs(fr))
    with pytest.raises(L.IvfError):
        SmoothGradVideo(smth_model, kind="mean")


def test_smoothgrad_video_clstm():
    import ivf_lib as L
    import ivf_recipe as RC
    from smoothgrad_videos import SmoothGradVideo
    model = _kth_clstm()
    x = torch.from_numpy(RC.clip(7, 3, 32, 120, 160))[None]
    sgv = SmoothGradVideo(model, n_samples=3, level=0.15, kind="sq", archType="CLSTM")
    m, out = sgv(x, index=2)
    assert m.shape == (32, 120, 160) and m.dtype == np.float32 and tuple(out.shape) == (1, 6)
    assert np.isfinite(m).all() and (m >= 0).all() and m.any()
    for k in ("sg_map", "sq_map", "var_map", "sg_frames", "sq_frames", "var_frames", "sample_scores", "sigma", "score_x"):
        assert k in sgv.last
    assert tuple(sgv.last["sample_scores"].shape) == (1, 3)
    with pytest.raises(L.IvfError):
        SmoothGradVideo(model, archType="VGG")(x)


def _check_sg_records(sg, tm, T, H, W, count, n, level, seed):
    assert len(sg) == len(tm) == count
    for rec, trec in zip(sg, tm):
        assert set(rec) == {'true_class', 'pred_class', 'video_id', 'SGHeatMap', 'SGSqHeatMap', 'SGVarHeatMap', 'SGFrames',
                            'sigma', 'n_samples', 'level', 'seed'}
        for k in ('SGHeatMap', 'SGSqHeatMap', 'SGVarHeatMap'):
            assert rec[k].shape == (T, H, W) and rec[k].dtype == np.float32 and np.isfinite(rec[k]).all()
        assert rec['SGFrames'].shape == (T,) and rec['pred_class'] == trec['pred_class']
        m = rec['SGHeatMap'].astype(F64)
        bound = sum_bound(np.abs(m).sum((1, 2)), H * W) + U * np.abs(rec['SGFrames'])
        assert np.all(np.abs(rec['SGFrames'] - m.sum((1, 2))) <= bound)
        assert (rec['SGHeatMap'] >= 0).all() and rec['SGHeatMap'].any() and (rec['SGSqHeatMap'] >= 0).all()
        assert isinstance(rec['sigma'], float) and rec['sigma'] > 0
        assert (rec['n_samples'], rec['level'], rec['seed']) == (n, level, seed)


def test_smth_driver_with_smoothgrad(smth_model, tmp_path, monkeypatch):
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(drv._state, "sub_dir", "run0")     # a driver's main() run earlier in the process leaves its own
    loader = ivf_find_masks.SyntheticLoader(2, 2, (3, 16, 224, 224), 174, first_id=40)
    hp = {"batch_size": 2, "gradCamType": "guessed"}
    drv.find_masks(loader, smth_model, hp, 0.01, 0.02, 2, "central", "freeze", classOI=None, doGradCam=False,
                   runTempMask=True, verbose=False, doSmoothGrad=True, sgSamples=2, sgLevel=0.1, sgSeed=5)
    tm = pickle.load(open(tmp_path / "results" / "allTimeMaskResults_run0_None_.p", "rb"))
    sg = pickle.load(open(tmp_path / "results" / "allSmoothGradResults_run0_None_.p", "rb"))
    _check_sg_records(sg, tm, 16, 224, 224, 2, 2, 0.1, 5)
    assert pickle.load(open(tmp_path / "results" / "allGradCamResults_run0_None_.p", "rb")) == []
    assert sg[0]['video_id'] == 40 and len(ivf_find_masks.find_masks_impl.last_sg_results) == 2
    strips = [p for p in (tmp_path / "cam_saved_images").rglob("smoothgrad/*.png")]
    assert any(p.name == "casefreeze40_15.png" for p in strips) and any(p.name == "casereverse41_0.png" for p in strips)
    assert len(list((tmp_path / "cam_saved_images").rglob("smoothgrad/mygif.gif"))) == 2


def test_kth_driver_with_smoothgrad_on_the_convlstm(tmp_path, monkeypatch):
    import FindMasksComparison_I3D_KTH as drv
    import ivf_find_masks
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    loader = ivf_find_masks.SyntheticLoader(1, 1, (3, 32, 120, 160), 6, first_id=7)
    drv.find_masks(loader, _kth_clstm(), {"batch_size": 1, "gradCamType": "guessed"}, 0.02, 0.04, 2, 1, "central",
                   "freeze", classOI=None, doGradCam=False, runTempMask=True, verbose=False, doSmoothGrad=True,
                   sgSamples=2)
    tm = pickle.load(open(tmp_path / "results" / "I3d_KTH_allTimeMaskResults_original_run0.p", "rb"))
    sg = pickle.load(open(tmp_path / "results" / "I3d_KTH_allSmoothGradResults_original_run0.p", "rb"))
    _check_sg_records(sg, tm, 32, 120, 160, 1, 2, 0.15, 0)
    assert sg[0]['video_id'] == "7"
    assert len(list((tmp_path / "cam_saved_images").rglob("smoothgrad/mygif.gif"))) == 1


def test_records_are_byte_identical_with_smoothgrad_off(smth_model, tmp_path, monkeypatch):
    import FindMasksComparison_I3D_smth as drv
    import ivf_find_masks
    monkeypatch.setitem(drv._state, "sub_dir", "run0")
    blobs = []
    for sub, extra in (("plain", {}), ("kwargs", dict(doSmoothGrad=False, sgSamples=7, sgLevel=0.3, sgSeed=9))):
        d = tmp_path / sub
        d.mkdir()
        monkeypatch.chdir(d)
        loader = ivf_find_masks.SyntheticLoader(1, 1, (3, 16, 224, 224), 174, first_id=40)
        drv.find_masks(loader, smth_model, {"batch_size": 1, "gradCamType": "guessed"}, 0.01, 0.02, 2, "central",
                       "freeze", classOI=None, doGradCam=True, runTempMask=True, verbose=False, **extra)
        files = sorted(p.relative_to(d) for p in d.rglob("*") if p.is_file())
        blobs.append({str(p): (d / p).read_bytes() for p in files})
        assert not any("SmoothGrad" in str(p) or "smoothgrad" in str(p) for p in files)
    assert blobs[0].keys() == blobs[1].keys()
    assert all(blobs[0][k] == blobs[1][k] for k in blobs[0]), [k for k in blobs[0] if blobs[0][k] != blobs[1][k]]


def test_tf_plan_refuses():
    import ivf_engine
    import ivf_lib as L
    eng = ivf_engine.TFCLSTMEngine(6, (1, 4, 30, 40), units=(4,), kernel=(3, 5), stride=2, padding="valid", max_batch=1)
    x = torch.zeros(1, 1, 4, 30, 40, device="cuda")
    with pytest.raises(L.IvfError):
        eng.smoothgrad(x, [0])
    with pytest.raises(L.IvfError):
        eng.sg_noise(1)
