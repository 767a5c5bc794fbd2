"""Case tables, seeded inputs, fp64 references, an fp32 emulation of the kernels' rounding and error bounds for
SmoothGrad / SmoothGrad^2 / VarGrad (csrc/smoothgrad_ops.hip; test_gpu_smoothgrad.py on the GPU,
test_sg_refs_host.py on the CPU).  Both files iterate the tables below.  Nothing here needs a GPU.

The method is an extension without a counterpart in the reference: these are numpy / torch fp64 restatements of the
semantics of DESIGN section 15, pinned by torch autograd on the reference's models, not reference output.

Rounding model: that of mask_refs (U = 2^-24, gamma(k) = k U / (1 - k U)).

Noise.  uint32 arithmetic restated in numpy uint64 masked to 32 bits (rise_refs.fmix32):
    key = fmix32(seed + 0x9E3779B9 (k + 1));  a = fmix32(key ^ (0x85EBCA77 (e + 1)))  (= rise_refs.hash_u(seed, k, e))
    h2 = fmix32(a + 0x9E3779B9);  u1 = (2 (a >> 9) + 1) 2^-24;  u2 = (h2 >> 8) 2^-24;  z = sqrt(-2 ln u1) cos(2 pi u2)
The fp64 reference takes cos(pi t), t = 2 u2, with the argument reduced exactly (t is a multiple of 2^-23), so it is
accurate relative to |z| also next to the zeros of the cosine.

Noise gate.  z32 = fl(fl(sqrt(fl(-2 fl(ln u1)))) * fl(cospi(2 u2))).  With every function correctly rounded (relative
error U each) the first-order sum is U/2 (log, halved by the root) + U (root) + U (cosine) + U (product) = 3.5 U; the
worst |z32 - z64| taken as the emulation's figure is 3.8 U |z| (`Z_EMULATION_C`; `z32` below measures 3.2 U |z| over
2^22 draws of each of the seeds 0, 1, 12345 -- the larger figure is kept).  The device functions are not correctly
rounded: the ROCm HIP math API reference lists a maximum error of 1 ulp each for logf, sqrtf and cospif.  One ulp is at
most 2^-23 = 2 U relative, so on top of the emulation the device may add 2 U / 2 (logf, halved by the root) + 2 U
(sqrtf) + 2 U (cospif):
    Z_GATE_C = 3.8 + 1 + 2 + 2 = 8.8,      |z_gpu - z64| <= Z_GATE_C U |z64|                       (`z_gate`)

Stage.  p = fmaf(sigma, z, x), one rounding: |p_gpu - p64| <= U |p64| + sigma Z_GATE_C U |z64|      (`stage_bound`).
At sigma == 0 the product is a signed zero and p == x bit for bit (for x != -0.0).

Accumulate.  G1 adds n times from +0.0 (the first add is exact): |G1_fp32 - G1| <= gamma(n) sum |g|.  G2 = fmaf(g, g, G2),
one rounding per sample: |G2_fp32 - G2| <= gamma(n) sum g^2 <= gamma(n + 1) sum g^2  (the issue's form).

Finish (every operation rounded once, c ascending from +0.0, sums of magnitudes, nothing clamped):
    sg term |fl(G1 / n)|: one rounding, then at most C adds:       b_sg  = gamma(C + 1) sum_c |G1_c| / n
    sq term fl(G2 / n) likewise:                                   b_sq  = gamma(C + 1) sum_c |G2_c| / n
    var term fl(fl(G2 - fl(G1 fl(G1 / n))) / (n - 1)): the product P = G1^2 / n carries two roundings, the difference
    one more on |d| <= |G2| + P, the division one more, then at most C adds:
                                                                   b_var = gamma(C + 4) sum_c (|G2_c| + G1_c^2 / n) / (n - 1)
    frames add the HW pixels in some fixed order (at most HW more roundings): the same with C + HW in place of C.

Chain (clstm_refs case S2, n = 4).  As ig_refs: the reference is torch fp64 autograd through clstm_refs' functional model
at the fp64 noisy points x + sigma z64; the floor of a tensor is elem_err of the SAME pipeline in float32 against it,
the gate GATE_MARGIN times that.  CHAIN_IDS are clips whose fp64 run has no ambiguous pool window on any sample row at
either level, so no clip is left out.
"""
import functools
import zlib
from collections import OrderedDict

import numpy as np
import torch

import clstm_refs as CR
import ig_refs as IGR
from leaf_refs import U
from mask_refs import gamma
from rise_refs import M32, fmix32, hash_u

F32, F64 = np.float32, np.float64
LAYOUTS = (0, 4)            # NCTHW, 16-byte channels-last pixels
Z_EMULATION_C = 3.8         # correctly rounded fp32 log, sqrt, cos and one product, worst over 2^22 draws
Z_GATE_C = Z_EMULATION_C + 1.0 + 2.0 + 2.0      # + logf (1 ulp, halved by the root), sqrtf (1 ulp), cospif (1 ulp)
Z_MAX = float(np.sqrt(48.0 * np.log(2.0)))      # u1 >= 2^-24

to_layout, from_layout, windows = IGR.to_layout, IGR.from_layout, IGR.windows


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------ noise
def hash_pair(seed, k, e):
    """(a, h2) as uint64 holding uint32; k and e broadcast"""
    a = hash_u(seed, k, e)
    return a, fmix32((a + np.uint64(0x9E3779B9)) & M32)


def uniforms(seed, k, e, mutant=None):
    """(u1 in (0,1), u2 in [0,1)) float64, both multiples of 2^-24 (exact in fp32).  mutant 'u2froma': u2 from a"""
    a, h2 = hash_pair(seed, k, e)
    if mutant == "u2froma":
        h2 = a
    u1 = (2.0 * (a >> np.uint64(9)).astype(F64) + 1.0) * 2.0 ** -24
    u2 = (h2 >> np.uint64(8)).astype(F64) * 2.0 ** -24
    return u1, u2


def cospi(t):
    """cos(pi t) in float64 for t in [0, 2) a multiple of 2^-23, the argument reduced exactly"""
    t = np.asarray(t, dtype=F64)
    r = np.where(t > 1.0, 2.0 - t, t)                   # cos(pi (2 - t)) = cos(pi t)
    neg = r > 0.5
    r = np.where(neg, 1.0 - r, r)                       # cos(pi (1 - r)) = -cos(pi r)
    c = np.where(r <= 0.25, np.cos(np.pi * r), np.sin(np.pi * (0.5 - r)))
    return np.where(neg, -c, c)


def z64(seed, k, e, mutant=None):
    u1, u2 = uniforms(seed, k, e, mutant)
    return np.sqrt(-2.0 * np.log(u1)) * cospi(2.0 * u2)


def z32(seed, k, e):
    """the kernel's formula with every operation correctly rounded to fp32 (computed in float64, rounded once each)"""
    u1, u2 = uniforms(seed, k, e)
    l = np.log(u1).astype(F32)
    s = np.sqrt((F32(-2.0) * l).astype(F64)).astype(F32)
    c = cospi(2.0 * u2).astype(F32)
    return (s * c).astype(F32)


def z32_cosf(seed, k, e):
    """the form the kernel does NOT use: cosf(fl(2 pi) * u2), whose argument error is absolute"""
    u1, u2 = uniforms(seed, k, e)
    s = np.sqrt((F32(-2.0) * np.log(u1).astype(F32)).astype(F64)).astype(F32)
    arg = (F32(6.2831853071795864769) * u2.astype(F32)).astype(F32)
    return (s * np.cos(arg.astype(F64)).astype(F32)).astype(F32)


def z_gate(z):
    return Z_GATE_C * U * np.abs(z)


def elem_index(C, T, HW, mutant=None):
    """e [C,T,HW] (uint64): the NCTHW index inside one clip; mutant 'clorder': the channels-last index"""
    c, t, px = np.meshgrid(np.arange(C), np.arange(T), np.arange(HW), indexing="ij")
    e = (t * HW + px) * C + c if mutant == "clorder" else (c * T + t) * HW + px
    return e.astype(np.uint64)


def noise(seed, ks, C, T, HW, mutant=None):
    """z64 [len(ks),C,T,HW].  mutants: 'samenoise' (every sample draws sample 0's), 'u2froma', 'clorder'"""
    ks = np.asarray(ks, dtype=np.uint64)
    if mutant == "samenoise":
        ks = np.zeros_like(ks)
    e = elem_index(C, T, HW, mutant)
    return z64(seed, ks.reshape(-1, 1, 1, 1), e[None], mutant)


# known answers: (seed, k, e) -> a (uint32), written down from this restatement once and checked against
# rise_refs.hash_u, which tests/test_rise_refs_host.py pins (`python tests/sg_refs.py` prints them)
HASH_CASES = ((0, 0, 0), (0, 1, 0), (1, 0, 1), (12345, 7, 385 * 3 * 5 - 1), (0xFFFFFFFF, 31, 2 ** 31 - 2),
              (12345, 0, 2 ** 31 - 2))


# ------------------------------------------------------------------------------------------------ range
def sigma_ref(x, level, mutant=None):
    """sigma [B] float32: one fp32 subtraction and one fp32 multiplication.  mutant 'maxonly': level * max"""
    v = np.asarray(x, dtype=F32).reshape(len(x), -1)
    hi, lo = v.max(1), v.min(1)
    d = hi if mutant == "maxonly" else (hi - lo).astype(F32)
    return (F32(level) * d).astype(F32)


def range_inputs(per_clip, B=3):
    """x [B, per_clip] fp32: clip 0 has its maximum in the last element, clip 1 its minimum in the last element of a
    non-multiple-of-4 tail (or the last element again), clip 2 both extremes inside"""
    x = _rng("range", per_clip, B).uniform(-3.0, 250.0, (B, per_clip)).astype(F32)
    x[0, -1] = F32(300.5)
    if B > 1:
        x[1, -1 if per_clip % 4 else -2] = F32(-77.25)
    return x


RANGE_SIZES = (1, 35, 1023, 1024, 1028, 4099, 385 * 3 * 5, 388 * 3 * 5)


# ------------------------------------------------------------------------------------------------ shapes
# (B, C, T, HW, n): the table of ig_refs with n samples for K nodes
STAGE_SHAPES = IGR.STAGE_SHAPES
ACC_SHAPES = IGR.ACC_SHAPES
SEED = 12345
LEVEL = 0.15


def stage_inputs(shape):
    """x [B,C,T,HW] fp32 in 40..255: the minimum is far from 0, so a sigma taken from the maximum alone is 19 % off"""
    B, C, T, HW, n = shape
    return _rng("sgstage", shape).uniform(40.0, 255.0, (B, C, T, HW)).astype(F32)


def stage_ref(x, sigma, z):
    """(p64 [B,n,C,T,HW], bound): x + sigma z64 and U |p| + sigma Z_GATE_C U |z|; z [n,C,T,HW] float64"""
    s = np.asarray(sigma, dtype=F32).astype(F64).reshape(-1, 1, 1, 1, 1)
    p = x.astype(F64)[:, None] + s * z[None]
    return p, U * np.abs(p) + s * z_gate(z)[None]


def stage_fp32(x, sigma, zf):
    """the kernel's own arithmetic on an fp32 z: fmaf(sigma, z, x) (ig_refs' note on double rounding applies)"""
    s = np.asarray(sigma, dtype=F32).astype(F64).reshape(-1, 1, 1, 1, 1)
    return (s * zf.astype(F64)[None] + x.astype(F64)[:, None]).astype(F32)


# ------------------------------------------------------------------------------------------------ accumulate / finish
def acc_inputs(shape):
    """din [B,n,C,T,HW] fp32: gradients of both signs whose size differs by sample, channel and clip (ig_refs)"""
    return IGR.acc_inputs(shape)[0]


def moments_ref(din):
    """(G1, G2 float64 [B,C,T,HW], bound1 = gamma(n) sum |g|, bound2 = gamma(n + 1) sum g^2)"""
    g = din.astype(F64)
    n = g.shape[1]
    return g.sum(1), (g * g).sum(1), gamma(n) * np.abs(g).sum(1), gamma(n + 1) * (g * g).sum(1)


def moments_fp32(din, mutant=None):
    """the kernel's own arithmetic: G1 = G1 + g, G2 = fmaf(g, g, G2), k ascending"""
    a1 = np.zeros(din[:, 0].shape, dtype=F32)
    a2 = np.zeros(din[:, 0].shape, dtype=F32)
    for k in range(din.shape[1]):
        g = din[:, k]
        a1 = (a1 + g).astype(F32)
        a2 = (g.astype(F64) * g.astype(F64) + a2.astype(F64)).astype(F32)
    if mutant == "g2fromg1":
        a2 = (a1 * a1).astype(F32)
    return a1, a2


def finish_ref(G1, G2, n, mutant=None):
    """fp64 finish of [B,C,T,HW] moments: dict of sg, sq, var [B,T,HW], their frame sums [B,T] and the bounds.
    mutants: 'dropchannel' (the last channel missing from the sums), 'divn' (n where n - 1 belongs)"""
    G1, G2 = np.asarray(G1, F64), np.asarray(G2, F64)
    if mutant == "dropchannel":
        G1, G2 = G1[:, :-1], G2[:, :-1]
    B, C, T, HW = G1.shape
    den = n if mutant == "divn" else n - 1
    out = {"sg": np.abs(G1 / n).sum(1), "sq": (G2 / n).sum(1)}
    out["var"] = ((G2 - G1 * (G1 / n)) / den).sum(1) if n > 1 else np.zeros((B, T, HW))
    mag = {"sg": np.abs(G1).sum(1) / n, "sq": np.abs(G2).sum(1) / n,
           "var": (np.abs(G2) + G1 * G1 / n).sum(1) / max(n - 1, 1)}
    extra = {"sg": 1, "sq": 1, "var": 4}
    for k in ("sg", "sq", "var"):
        out[f"{k}_frames"] = out[k].sum(2)
        out[f"b_{k}"] = gamma(C + extra[k]) * mag[k]
        out[f"b_{k}_frames"] = gamma(C + extra[k] + HW) * mag[k].sum(2)
    return out


def finish_fp32(G1, G2, n):
    """the kernel's own arithmetic in numpy float32 (each operation rounded once); frames in pixel order, one of the
    fixed orders the bound covers"""
    G1, G2 = np.asarray(G1, F32), np.asarray(G2, F32)
    B, C, T, HW = G1.shape
    nf, nm1 = F32(n), F32(n - 1)
    sg, sq, var = (np.zeros((B, T, HW), F32) for _ in range(3))
    for c in range(C):
        m = (G1[:, c] / nf).astype(F32)
        sg = (sg + np.abs(m)).astype(F32)
        sq = (sq + (G2[:, c] / nf).astype(F32)).astype(F32)
        if n > 1:
            d = (G2[:, c] - (G1[:, c] * m).astype(F32)).astype(F32)
            var = (var + (d / nm1).astype(F32)).astype(F32)
    out = {"sg": sg, "sq": sq, "var": var}
    for k in ("sg", "sq", "var"):
        fr = np.zeros((B, T), F32)
        for px in range(HW):
            fr = (fr + out[k][:, :, px]).astype(F32)
        out[f"{k}_frames"] = fr
    return out


def cancellation(var_map, G2, n):
    """sum var_map (n - 1) / sum G2: 1 where the gradients of the samples are unrelated, -> 0 where they agree"""
    return float(np.sum(np.asarray(var_map, F64)) * (n - 1) / np.sum(np.asarray(G2, F64)))


# ------------------------------------------------------------------------------------------------ the whole method
TENSORS = ("sg", "sq", "var", "sg_frames", "sq_frames", "var_frames", "sample_scores")


def sg_pipeline(x, sigma, z, grad_fn, dtype=F64, mutant=None):
    """The method in `dtype` (numpy): x [B,C,T,H,W], sigma [B], z [n,C,T,H,W]; grad_fn(points [B*n,C,T,H,W] as `dtype`)
    -> (score [B*n], d score / d point).  Returns float64 arrays: sg, sq, var [B,T,H,W], *_frames [B,T], sample_scores
    [B,n], G1, G2 and the points."""
    B, C, T, H, W = x.shape
    n = len(z)
    s = np.asarray(sigma, dtype=F32).astype(dtype).reshape(B, 1, 1, 1, 1, 1)
    pts = (x.astype(dtype)[:, None] + s * z.astype(dtype)[None]).astype(dtype).reshape(B * n, C, T, H, W)
    score, g = grad_fn(pts)
    g = np.asarray(g).reshape(B, n, C, T, H, W).astype(dtype)
    G1 = np.zeros(x.shape, dtype=dtype)
    G2 = np.zeros(x.shape, dtype=dtype)
    for k in range(n):
        G1 = (G1 + g[:, k]).astype(dtype)
        G2 = (G2 + g[:, k] * g[:, k]).astype(dtype)
    if mutant == "g2fromg1":
        G2 = G1 * G1
    nd = np.asarray(n, dtype=dtype)
    A1, A2 = (G1, G2) if mutant != "dropchannel" else (G1[:, :-1], G2[:, :-1])
    den = nd if mutant == "divn" else nd - 1
    out = {"sg": np.abs(A1 / nd).sum(1, dtype=dtype), "sq": (A2 / nd).sum(1, dtype=dtype)}
    out["var"] = ((A2 - A1 * (A1 / nd)) / den).sum(1, dtype=dtype) if n > 1 else np.zeros((B, T, H, W), dtype)
    for k in ("sg", "sq", "var"):
        out[f"{k}_frames"] = out[k].sum((2, 3), dtype=dtype)
    out = {k: np.asarray(v, F64) for k, v in out.items()}
    out.update(sample_scores=np.asarray(score, F64).reshape(B, n), G1=G1.astype(F64), G2=G2.astype(F64), points=pts)
    return out


# ------------------------------------------------------------------------------------------------ chain (ConvLSTM S2)
CHAIN_CASE = "S2"
CHAIN_N = 4
CHAIN_LEVELS = (0.05, 0.15)
CHAIN_SEED = 0
# the first ids from the case's id0 on whose fp64 run has no ambiguous pool window on any sample row at either level
# (`python tests/sg_refs.py` prints them; test_sg_refs_host.py asserts it)
CHAIN_IDS = (200, 201)
MUTANTS = ("samenoise", "u2froma", "maxonly", "g2fromg1", "dropchannel", "divn", "clorder")


def chain_inputs(ids=None):
    case = CR.CASES[CHAIN_CASE]
    ids = CHAIN_IDS if ids is None else ids
    _, sd, _, _ = CR.case_inputs(case)
    x = CR.clips(case, ids)
    targets = [r % CR.K for r in range(len(ids))]
    return case, x, sd, targets


def _chain_run(case, x, sd, targets, level, dtype, mutant=None, keep=None):
    B, C, T, H, W = x.shape
    z = noise(CHAIN_SEED, range(CHAIN_N), C, T, H * W, mutant).reshape(CHAIN_N, C, T, H, W)
    sigma = sigma_ref(x, level, mutant)
    return sg_pipeline(x, sigma, z, IGR._chain_grad_fn(case, sd, targets, CHAIN_N, {F64: torch.float64,
                                                                                   F32: torch.float32}[dtype], keep),
                       dtype, mutant)


@functools.lru_cache(maxsize=None)
def chain_reference(level, ids=None):
    """Everything both tests need of the chain case at one level: inputs, the fp64 method, the float32 floor and gate
    per tensor, and the ambiguous pool windows per sample row."""
    case, x, sd, targets = chain_inputs(ids)
    runs = []
    ref = _chain_run(case, x, sd, targets, level, F64, keep=runs)
    f32 = _chain_run(case, x, sd, targets, level, F32)
    floor = OrderedDict((n, max(U, float(np.max(IGR.chain_err(f32[n], ref[n]))))) for n in TENSORS)
    fl, _ = CR.floors(case, torch.from_numpy(ref["points"]), sd, runs[0], backward=False)
    amb, ties = CR.ambiguous_windows(runs[0]["pre"], fl)
    return {"case": case, "x": x, "sd": sd, "targets": targets, "level": level, "ref": ref, "f32": f32, "floor": floor,
            "gate": OrderedDict((n, CR.GATE_MARGIN * v) for n, v in floor.items()), "ambiguous": amb, "ties": ties}


def chain_mutant(bundle, mutant):
    return _chain_run(bundle["case"], bundle["x"], bundle["sd"], bundle["targets"], bundle["level"], F64, mutant)


def pick_chain_ids(n=2, limit=400):
    case = CR.CASES[CHAIN_CASE]
    ids = []
    for i in range(case.id0, case.id0 + limit):
        if all(int(chain_reference.__wrapped__(lv, (i,))["ambiguous"].sum()) == 0 for lv in CHAIN_LEVELS):
            ids.append(i)
        if len(ids) == n:
            break
    return tuple(ids)


# ------------------------------------------------------------------------------------------------ I3D fixture gates
I3D_L2_GATE, I3D_MAX_GATE, I3D_EXACT, I3D_CLIPS = IGR.I3D_L2_GATE, IGR.I3D_MAX_GATE, IGR.I3D_EXACT, IGR.I3D_CLIPS
I3D_N, I3D_LEVEL, I3D_SEED = 8, 0.15, 0
# var_map is held against the fixture's own spread: the gate is LEG_FACTOR times the larger distance of the fp64 and
# 4-thread legs from the fp32 leg -- the IG fixture's legs sit inside half its gates, i.e. its gates are at least twice
# its spread (test_ig_refs_host.py::test_fixture_noise_floor_is_inside_half_the_gate)
LEG_FACTOR = 2.0


def i3d_var_gates(g, cid):
    """(L2 gate, max gate) of the sampled var_map of clip `cid` from the fixture's legs"""
    ref = g[f"c{cid}_var_val"]
    l2 = max(np.linalg.norm(g[f"{leg}_c{cid}_var_val"] - ref) / np.linalg.norm(ref) for leg in ("f64", "f32t4"))
    mx = max(np.max(np.abs(g[f"{leg}_c{cid}_var_val"] - ref)) / np.max(np.abs(ref)) for leg in ("f64", "f32t4"))
    return LEG_FACTOR * float(l2), LEG_FACTOR * float(mx)


if __name__ == "__main__":
    for s, k, e in HASH_CASES:
        print((s, k, e), int(hash_u(s, k, e)), float(z64(s, k, e)))
    print("CHAIN_IDS =", pick_chain_ids())
