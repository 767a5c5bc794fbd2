"""CPU test of tests/sg_refs.py and of the host side of csrc/smoothgrad_ops.hip: the noise hash against a pinned hash
and known answers, the uniforms, the statistics of the noise, the fp64 pipeline against torch autograd, every bound used
on the GPU against an emulation of the kernels' own fp32 arithmetic, what wrong implementations would do to the gates,
the fixture's own noise floor, and the argument checks of the new entries -- on the very inputs
test_gpu_smoothgrad.py later runs the kernels on.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import ig_refs as IGR
import rise_refs as RR
import sg_refs as R
from conftest import GOLDEN, note
from leaf_refs import U

F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------- (a) hash, uniforms
def _fmix_int(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


KNOWN_A = {(0, 0, 0): 1624822673, (0, 1, 0): 2966535489, (1, 0, 1): 3521136143, (12345, 7, 385 * 3 * 5 - 1): 2404669328,
           (0xFFFFFFFF, 31, 2 ** 31 - 2): 2310570641, (12345, 0, 2 ** 31 - 2): 31639510}


def test_hash_is_the_rise_cell_hash_and_known_answers():
    """a(seed, k, e) == rise_refs.hash_u with e for the cell (pinned by test_rise_refs_host.py), == plain Python
    integers, == the written-down answers, e = 2^31 - 2 included (e + 1 = 2^31 - 1, the largest allowed)"""
    assert set(KNOWN_A) == set(R.HASH_CASES)
    for (seed, k, e), want in KNOWN_A.items():
        a, h2 = R.hash_pair(seed, k, e)
        key = _fmix_int((seed + 0x9E3779B9 * (k + 1)) & 0xFFFFFFFF)
        ai = _fmix_int(key ^ ((0x85EBCA77 * (e + 1)) & 0xFFFFFFFF))
        assert int(a) == int(RR.hash_u(seed, k, e)) == ai == want, (seed, k, e)
        assert int(h2) == _fmix_int((ai + 0x9E3779B9) & 0xFFFFFFFF)
    g = np.random.default_rng(5)
    k, e = g.integers(0, 1000, 4096), g.integers(0, 2 ** 31 - 1, 4096)
    assert np.array_equal(R.hash_pair(77, k, e)[0], RR.hash_u(77, k, e))


def test_uniforms_are_exact_in_fp32_and_inside_their_ranges():
    e = np.arange(1 << 18, dtype=np.uint64)
    for seed in (0, 1, 12345):
        u1, u2 = R.uniforms(seed, 3, e)
        assert np.array_equal(u1.astype(F32).astype(F64), u1) and np.array_equal(u2.astype(F32).astype(F64), u2)
        assert u1.min() > 0.0 and u1.max() < 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    # the edges of the construction itself
    assert (2.0 * 0 + 1.0) * 2.0 ** -24 > 0 and (2.0 * (2 ** 23 - 1) + 1.0) * 2.0 ** -24 < 1
    assert F32((2 ** 24 - 1) * 2.0 ** -24) < F32(1.0)
    assert abs(np.sqrt(-2.0 * np.log(2.0 ** -24)) - R.Z_MAX) < 1e-12 and abs(R.Z_MAX - 5.768) < 1e-3
    # cospi: exact zeros and signs at the quarter points, where cos(2 pi u2) in float64 would leave 6e-17
    assert np.array_equal(R.cospi(np.array([0.0, 0.5, 1.0, 1.5])), np.array([1.0, 0.0, -1.0, 0.0]))
    t = np.arange(0, 2, 2.0 ** -10)
    assert np.max(np.abs(R.cospi(t) - np.cos(np.pi * t))) < 1e-15


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_noise_statistics(seed):
    """N = 2^22 draws: mean, variance, fourth moment, lag-1 correlation over e, correlation between two samples and
    lag-1 correlation of z^2, each within 5 of its standard error; and the fp32 emulation's floor"""
    N = 1 << 22
    e = np.arange(N, dtype=np.uint64)
    z, z1 = R.z64(seed, 0, e), R.z64(seed, 1, e)
    figs = {"mean": z.mean() / np.sqrt(1.0 / N), "variance": (z.var() - 1.0) / np.sqrt(2.0 / N),
            "fourth moment": ((z ** 4).mean() - 3.0) / np.sqrt(96.0 / N),
            "lag-1 over e": (z[:-1] * z[1:]).mean() / np.sqrt(1.0 / N),
            "between samples": (z * z1).mean() / np.sqrt(1.0 / N),
            "lag-1 of z^2": np.corrcoef(z[:-1] ** 2, z[1:] ** 2)[0, 1] / np.sqrt(1.0 / N)}
    note(f"sg noise seed {seed}: " + ", ".join(f"{k} {v:+.2f} se" for k, v in figs.items()))
    for k, v in figs.items():
        assert abs(v) <= 5.0, (seed, k, v)
    assert np.abs(z).max() <= R.Z_MAX
    zf = R.z32(seed, 0, e)
    nz = z != 0
    ratio = float(np.max(np.abs(zf.astype(F64) - z)[nz] / (U * np.abs(z[nz]))))
    note(f"sg noise seed {seed}: correctly rounded fp32 emulation worst |z32 - z64| = {ratio:.2f} U |z| "
         f"(Z_EMULATION_C {R.Z_EMULATION_C}, gate {R.Z_GATE_C})")
    assert ratio <= R.Z_EMULATION_C and np.array_equal(zf[~nz], z[~nz].astype(F32))
    if seed == 0:
        zc = R.z32_cosf(seed, 0, e[:1 << 20])
        bad = float(np.max(np.abs(zc.astype(F64) - z[:1 << 20]))) / U
        note(f"sg noise: the cosf(2 pi u2) form is off by {bad:.1f} U absolute, whatever |z|")
        assert bad > R.Z_GATE_C          # it is an absolute error: next to a zero of the cosine no multiple of |z| covers it
        assert np.max(np.abs(zc.astype(F64) - z[:1 << 20]) / np.maximum(R.z_gate(z[:1 << 20]), 1e-300)) > 1.0


# ---------------------------------------------------------------------------------------------------- (b) the reference
def test_pipeline_equals_torch_autograd_on_a_smooth_function():
    """On f(p) = a.p + p.Q p with explicit noise: G1, G2 and the three maps of the fp64 pipeline equal what torch autograd
    gives sample by sample; n = 1, level = 0 is the plain gradient map"""
    g = np.random.default_rng(3)
    B, C, T, H, W, n = 2, 2, 3, 2, 3, 5
    d = C * T * H * W
    a, Q = torch.from_numpy(g.normal(size=d)), torch.from_numpy(g.normal(size=(d, d)) / d)
    x = g.uniform(0, 1, (B, C, T, H, W)).astype(F32)

    def grad_fn(pts):
        p = torch.from_numpy(np.ascontiguousarray(pts)).requires_grad_()
        q = p.reshape(len(p), -1)
        s = q @ a + ((q @ Q) * q).sum(1)
        s.sum().backward()
        return s.detach().numpy(), p.grad.numpy()

    z = R.noise(9, range(n), C, T, H * W).reshape(n, C, T, H, W)
    sigma = R.sigma_ref(x, 0.15)
    assert np.array_equal(sigma, (F32(0.15) * (x.reshape(B, -1).max(1) - x.reshape(B, -1).min(1))).astype(F32))
    out = R.sg_pipeline(x, sigma, z, grad_fn)
    grads = []
    for b in range(B):
        for k in range(n):
            p = torch.from_numpy(x[b].astype(F64) + float(sigma[b]) * z[k]).requires_grad_()
            q = p.reshape(-1)
            (q @ a + (q @ Q) @ q).backward()
            grads.append(p.grad.numpy())
    gr = np.stack(grads).reshape(B, n, C, T, H, W)
    mean = gr.mean(1)
    assert np.allclose(out["sg"], np.abs(mean).sum(1), rtol=1e-12, atol=0)
    assert np.allclose(out["sq"], (gr ** 2).mean(1).sum(1), rtol=1e-12, atol=0)
    assert np.allclose(out["var"], gr.var(1, ddof=1).sum(1), rtol=1e-9, atol=1e-18)
    assert np.allclose(out["sg_frames"], out["sg"].sum((2, 3)), rtol=1e-13, atol=0)
    plain = R.sg_pipeline(x, R.sigma_ref(x, 0.0), z[:1], grad_fn)
    _, g0 = grad_fn(x.astype(F64))
    assert np.array_equal(plain["sg"], np.abs(g0).sum(1)) and not plain["var"].any()
    assert np.array_equal(plain["points"].reshape(x.shape), x.astype(F64))


# ---------------------------------------------------------------------------------------------------- (c) the bounds
def test_stage_bound_holds_for_the_kernel_arithmetic():
    worst = 0.0
    for shape in R.STAGE_SHAPES[::7]:
        B, C, T, HW, n = shape
        x = R.stage_inputs(shape)
        sigma = R.sigma_ref(x, R.LEVEL)
        e = R.elem_index(C, T, HW)
        ks = np.arange(n, dtype=np.uint64).reshape(-1, 1, 1, 1)
        z, zf = R.noise(R.SEED, range(n), C, T, HW), R.z32(R.SEED, ks, e[None])
        assert np.all(np.abs(zf.astype(F64) - z) <= R.z_gate(z))
        ref, bound = R.stage_ref(x, sigma, z)
        err = np.abs(R.stage_fp32(x, sigma, zf).astype(F64) - ref)
        assert np.all(err <= bound)
        worst = max(worst, float(np.max(err / bound)))
        assert np.array_equal(R.stage_fp32(x, R.sigma_ref(x, 0.0), zf), np.broadcast_to(x[:, None], ref.shape))
    note(f"sg stage: fp32 emulation uses {worst:.2f} of the U |p| + sigma (z gate) bound")
    assert worst > 0.05


@pytest.mark.parametrize("shape", R.ACC_SHAPES, ids=[str(s) for s in R.ACC_SHAPES])
def test_accumulate_and_finish_bounds_hold_for_fp32(shape):
    B, C, T, HW, n = shape
    din = R.acc_inputs(shape)
    G1, G2, b1, b2 = R.moments_ref(din)
    a1, a2 = R.moments_fp32(din)
    assert np.all(np.abs(a1.astype(F64) - G1) <= b1) and np.all(np.abs(a2.astype(F64) - G2) <= b2)
    f, got = R.finish_ref(a1, a2, n), R.finish_fp32(a1, a2, n)
    for k in ("sg", "sq", "var", "sg_frames", "sq_frames", "var_frames"):
        err = np.abs(got[k].astype(F64) - f[k])
        assert np.all(err <= f[f"b_{k}"]), (shape, k, float(np.max(err / np.maximum(f[f"b_{k}"], 1e-300))))
    if n == 1:
        assert not got["var"].any() and not f["var"].any()
    else:
        note(f"sg finish {shape}: sum var (n - 1) / sum G2 = {R.cancellation(f['var'], a2, n):.3f}")


def test_windows_cover_the_required_geometry():
    for B, n in ((1, 1), (1, 8), (3, 1), (3, 3), (3, 8)):
        ws = R.windows(B, n)
        assert ws[0] == (0, B * n)
        if B == 3:
            assert any({(first + j) // n for j in range(count)} == {0, 1, 2} and (n == 1 or first % n != 0)
                       for first, count in ws)
    assert {s[3] for s in R.STAGE_SHAPES} == {35, 385, 388} and {s[4] for s in R.STAGE_SHAPES} == {1, 3, 8}


def test_kernel_mutants_leave_the_bounds():
    """the noise of another sample, u2 from a, the channels-last element index, sigma from max alone: far outside the
    stage bound; G2 from G1^2, a dropped channel, n for n - 1: far outside the finish bounds"""
    shape = (3, 3, 5, 385, 3)
    B, C, T, HW, n = shape
    x = R.stage_inputs(shape)
    sigma = R.sigma_ref(x, R.LEVEL)
    z = R.noise(R.SEED, range(n), C, T, HW)
    ref, bound = R.stage_ref(x, sigma, z)
    for mutant in ("samenoise", "u2froma", "clorder", "maxonly"):
        zm = R.noise(R.SEED, range(n), C, T, HW, mutant)
        wrong, _ = R.stage_ref(x, R.sigma_ref(x, R.LEVEL, mutant), zm)
        rows = slice(1, None) if mutant == "samenoise" else slice(None)          # sample 0 is its own noise
        far = np.abs(wrong - ref)[:, rows] > 100 * bound[:, rows]
        note(f"sg stage mutant {mutant}: {far.mean():.3f} of the elements beyond 100 bounds")
        assert far.mean() > 0.9, mutant
    din = R.acc_inputs(shape)
    a1, a2 = R.moments_fp32(din)
    f = R.finish_ref(a1, a2, n)
    for mutant, keys in (("g2fromg1", ("sq", "var")), ("dropchannel", ("sg", "sq", "var")), ("divn", ("var",))):
        m1, m2 = R.moments_fp32(din, mutant)
        w = R.finish_ref(m1, m2, n, mutant if mutant != "g2fromg1" else None)
        for k in keys:
            far = np.abs(w[k] - f[k]) > 100 * f[f"b_{k}"]
            note(f"sg finish mutant {mutant} {k}: {far.mean():.3f} of the elements beyond 100 bounds")
            assert far.mean() > 0.9, (mutant, k)


# ---------------------------------------------------------------------------------------------------- (d) the chain case
@pytest.mark.parametrize("level", R.CHAIN_LEVELS)
def test_chain_has_no_ambiguous_window_on_any_sample_row(level):
    b = R.chain_reference(level)
    assert b["ambiguous"].shape == (len(R.CHAIN_IDS) * R.CHAIN_N,)
    assert int(b["ambiguous"].sum()) == 0, b["ambiguous"]
    for n in R.TENSORS:
        note(f"sg chain level {level} {n}: float32 floor {b['floor'][n]:.3e}, gate {b['gate'][n]:.3e}")
    note(f"sg chain level {level}: sum var (n - 1) / sum G2 = "
         f"{R.cancellation(b['ref']['var'], b['ref']['G2'], R.CHAIN_N):.4f}, sample scores "
         f"{b['ref']['sample_scores'].tolist()}")


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_chain_mutants_land_many_gates_away(mutant):
    """each mutant's distance in gates on the tensors it touches (the least over the clips)"""
    touched = {"samenoise": ("sg", "sq", "var"), "u2froma": ("sg", "sq", "var"), "clorder": ("sg", "sq", "var"),
               "maxonly": ("sg", "sq", "var"), "g2fromg1": ("sq", "var"), "dropchannel": ("sg", "sq", "var"),
               "divn": ("var",)}[mutant]
    for level in R.CHAIN_LEVELS:
        b = R.chain_reference(level)
        assert b["case"].C > 1                                       # a channel can be dropped
        out = R.chain_mutant(b, mutant)
        ratios = {n: float(np.min(IGR.chain_err(out[n], b["ref"][n]))) / b["gate"][n] for n in touched}
        note(f"sg chain level {level} mutant {mutant}: " + ", ".join(f"{n} {v:.1f} gates" for n, v in ratios.items()))
        assert max(ratios.values()) > 10, (level, mutant, ratios)


# ---------------------------------------------------------------------------------------------------- (e) the I3D fixture
def test_fixture_legs_are_inside_half_the_gates():
    """The fixture's fp64 and 4-thread runs against its fp32 / 8-thread run: sampled sg_map and sq_map inside half the
    whole-chain gates, frames inside half the gate times their magnitude sums (all three are sums of non-negative
    terms but var), sample scores inside half of 1e-3.  var_map's gate IS the spread (sg_refs.i3d_var_gates), so the legs
    sit at 1 / LEG_FACTOR of it by construction; the spread and the cancellation figure are recorded."""
    g = dict(np.load(os.path.join(GOLDEN, "smoothgrad.npz")))
    assert int(g["n"]) == R.I3D_N and float(g["level"]) == R.I3D_LEVEL and tuple(g["clips"]) == R.I3D_CLIPS
    l2_gate, max_gate = R.I3D_L2_GATE[True], R.I3D_MAX_GATE[True]
    for cid in R.I3D_CLIPS:
        p = f"c{cid}"
        for leg in ("f64", "f32t4"):
            q = f"{leg}_{p}"
            for k in ("sg", "sq"):
                ref = g[f"{p}_{k}_val"]
                l2 = np.linalg.norm(g[f"{q}_{k}_val"] - ref) / np.linalg.norm(ref)
                mx = np.max(np.abs(g[f"{q}_{k}_val"] - ref)) / np.max(np.abs(ref))
                ef = np.max(np.abs(g[f"{q}_{k}_frames"] - g[f"{p}_{k}_frames"]) / g[f"{p}_{k}_frames"])
                note(f"sg fixture {p} {leg} {k}: map L2 {l2:.2e} max {mx:.2e}, frames {ef:.2e}")
                assert l2 <= 0.5 * l2_gate and mx <= 0.5 * max_gate and ef <= 0.5 * l2_gate
            es = np.max(np.abs(g[f"{q}_sample_scores"] - g[f"{p}_sample_scores"]) / np.abs(g[f"{p}_sample_scores"]))
            evf = np.max(np.abs(g[f"{q}_var_frames"] - g[f"{p}_var_frames"]) / g[f"{p}_sq_frames"])
            note(f"sg fixture {p} {leg}: sample scores {es:.2e}, var_frames / sq_frames {evf:.2e}")
            assert es <= 0.5e-3 and evf <= 0.5 * l2_gate
        gl2, gmx = R.i3d_var_gates(g, cid)
        note(f"sg fixture {p}: var_map gates from the legs' spread (x{R.LEG_FACTOR:g}): L2 {gl2:.2e} max {gmx:.2e}; "
             f"sum var (n - 1) / sum G2 = {float(g[f'{p}_cancellation']):.4f}, sigma {float(g[f'{p}_sigma']):.4f}")
        assert 0 < gl2 and 0 < gmx


# ---------------------------------------------------------------------------------------------------- (f) argument checks
def test_workspace_is_the_sum_of_its_pieces():
    import ivf_lib as L
    lib = L.lib()

    def up(v):
        return (v + 255) // 256 * 256
    for b, C, T, HW, n in ((1, 1, 1, 1, 1), (2, 3, 16, 224 * 224, 32), (3, 1, 32, 120 * 160, 8), (5, 3, 17, 385, 3)):
        per = b * C * T * HW * 4
        assert lib.ivf_sg_workspace_bytes(b, C, T, HW, n) == 2 * up(per) + up(b * 4) + 2 * up(b * n * 4), (b, C, T, HW, n)
    assert lib.ivf_sg_workspace_bytes(0, 3, 4, 10, 2) == 0 and b"sg_workspace_bytes" in lib.ivf_last_error()
    assert lib.ivf_sg_workspace_bytes(1, 3, 4, 10, 0) == 0
    assert lib.ivf_sg_workspace_bytes(1, 3, 64, 2 ** 24, 1) == 0          # C T HW > 2^31 - 1


def test_bad_arguments_return_error_codes():
    import ivf_lib as L
    lib = L.lib()
    one = ctypes.c_void_p(256)          # a non-null address that is never dereferenced: every call below is refused
    odd = ctypes.c_void_p(260)
    nan, inf = float("nan"), float("inf")
    assert lib.ivf_sg_noise(0, 0, 1, 3, 4, 10, None, None) == -1 and b"sg_noise" in lib.ivf_last_error()
    assert lib.ivf_sg_noise(0, 0, 0, 3, 4, 10, one, None) == -1                       # no samples
    assert lib.ivf_sg_noise(0, -1, 1, 3, 4, 10, one, None) == -1
    assert lib.ivf_sg_noise(0, 0, 1, 3, 64, 2 ** 24, one, None) == -1                 # C T HW > 2^31 - 1
    assert lib.ivf_sg_range(None, 1, 3, 4, 10, 0.1, None, None) == -1 and b"sg_range" in lib.ivf_last_error()
    for level in (-0.1, nan, inf):
        assert lib.ivf_sg_range(one, 1, 3, 4, 10, level, one, None) == -1, level
    assert lib.ivf_sg_range(one, 0, 3, 4, 10, 0.1, one, None) == -1
    assert lib.ivf_sg_stage(None, None, 1, 3, 4, 10, 2, 0, 0, 1, None, 0, None) == -1 and b"sg_stage" in lib.ivf_last_error()
    assert lib.ivf_sg_stage(one, one, 1, 3, 4, 10, 0, 0, 0, 1, one, 0, None) == -1      # n
    assert lib.ivf_sg_stage(one, one, 1, 3, 4, 10, 2, 0, 1, 2, one, 0, None) == -1      # rows past b*n
    assert lib.ivf_sg_stage(one, one, 1, 3, 4, 10, 2, 0, -1, 1, one, 0, None) == -1
    assert lib.ivf_sg_stage(one, one, 1, 5, 4, 10, 2, 0, 0, 1, one, 4, None) == -1      # C > 4 channels-last
    assert lib.ivf_sg_stage(one, one, 1, 3, 4, 10, 2, 0, 0, 1, one, 8, None) == -1      # layout
    assert lib.ivf_sg_stage(one, one, 1, 3, 4, 10, 2, 0, 0, 1, odd, 4, None) == -1      # alignment
    assert lib.ivf_sg_accumulate(None, 0, 2, 0, 1, None, None, 1, 3, 4, 10, None) == -1
    assert b"sg_accumulate" in lib.ivf_last_error()
    assert lib.ivf_sg_accumulate(one, 0, 2, 2, 1, one, one, 1, 3, 4, 10, None) == -1    # rows past b*n
    assert lib.ivf_sg_accumulate(one, 4, 2, 0, 1, one, one, 1, 5, 4, 10, None) == -1    # C > 4 channels-last
    assert lib.ivf_sg_accumulate(odd, 4, 2, 0, 1, one, one, 1, 3, 4, 10, None) == -1    # alignment
    assert lib.ivf_sg_finish(None, None, 2, 1, 3, 4, 10, *([None] * 7)) == -1 and b"sg_finish" in lib.ivf_last_error()
    assert lib.ivf_sg_finish(one, one, 0, 1, 3, 4, 10, *([one] * 6), None) == -1        # n
    assert lib.ivf_sg_finish(one, one, 2, 1, 0, 4, 10, *([one] * 6), None) == -1        # dims
    for pfx in ("i3d", "clstm"):
        assert getattr(lib, f"ivf_{pfx}_smoothgrad")(None, None, 1, None, 4, 0.15, 0, *([None] * 10)) != 0
    assert not hasattr(lib, "ivf_tfclstm_smoothgrad")
