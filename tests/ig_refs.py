"""Case tables, seeded inputs, fp64 references and error bounds for Integrated Gradients (csrc/ig_ops.hip, DESIGN 13;
test_gpu_ig.py on the GPU, test_ig_refs_host.py on the CPU).  Both files iterate the tables below.  Nothing here needs
a GPU.

IG is an extension without a counterpart in the reference: these references are numpy / torch fp64
restatements of the semantics of DESIGN section 13, pinned by torch autograd on the reference's models, not reference
output.

Rounding model: that of mask_refs (U = 2^-24, gamma(k) = k U / (1 - k U)).

Stage.  v = fmaf(alpha, x - x0, x0): d = (x - x0)(1 + e1), v = (x0 + alpha d)(1 + e2), |e| <= U.  So
|v_fp32 - v| <= alpha |x - x0| U (1 + U) + |v| U.  For alpha in [0,1], v lies between x0 and x, |v| <= max(|x|, |x0|) = m,
and |x - x0| <= 2 m: the error is at most 3 U (1 + U) m < gamma(3) m             (`stage_bound`).
Where x == x0 the product is a signed zero and v == x0; at alpha == 0 likewise: both are bit-exact.

Accumulate.  acc_k = fmaf(w_k, g_k, acc_{k-1}) from +0.0: one rounding per node, a term passes through at most K of
them: |Gsum_fp32 - Gsum| <= gamma(K) sum_k |w_k g_k| <= gamma(K + 1) sum_k |w_k g_k|   (`gsum_bound`, the issue's form).

Finish.  A_c = (x - x0) Gsum is rounded twice (difference, product); ig_map adds C - 1 times:
    b_map = gamma(C + 1) sum_c |A_c|.
frames adds the HW pixels in some fixed order (at most HW - 1 more additions), abs_frames likewise, total T - 1 more:
    b_frames = gamma(C + HW) sum_{px,c} |A|,  b_total = gamma(C + HW + T) sum_{t,px,c} |A|       (any order).
With the 'frozen' baseline frame 0 has x == x0: every A is a signed zero and map, frames and abs_frames are 0.0 exactly.

Chain (clstm_refs case S2, K = 4).  The reference is torch fp64 autograd through clstm_refs' functional model at the
fp64 path points; the floor of a tensor is elem_err of the SAME pipeline in float32 against it (what a correct float32
implementation loses), the gate GATE_MARGIN times that, as for every tensor of clstm_refs.  CHAIN_IDS are clips whose
fp64 run has no ambiguous pool window at any path point of either baseline, so no clip is left out.
"""
import functools
import zlib
from collections import OrderedDict

import numpy as np
import torch

import clstm_refs as CR
from leaf_refs import U
from mask_refs import gamma

F32, F64 = np.float32, np.float64
FROZEN, CONSTANT, CLIP = 0, 1, 2
KINDS = OrderedDict((("frozen", FROZEN), ("constant", CONSTANT), ("clip", CLIP)))
LAYOUTS = (0, 4)            # NCTHW, 16-byte channels-last pixels


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def midpoint(K):
    """the default rule, built in fp32 as the engine builds it"""
    alpha = (2.0 * np.arange(K, dtype=F32) + F32(1.0)) / F32(2 * K)
    return alpha.astype(F32), np.full(K, F32(1.0) / F32(K), dtype=F32)


def left_riemann(K):
    return (np.arange(K, dtype=F32) / F32(K)).astype(F32), np.full(K, F32(1.0) / F32(K), dtype=F32)


# ------------------------------------------------------------------------------------------------ shapes
# (B, C, T, HW, K).  HW 35 and 385 are no multiple of 64 or 4 (the per-pixel NCTHW kernel, ragged last wave); 388 is a
# multiple of 4 and takes the 16-byte NCTHW kernel.
STAGE_SHAPES = [(B, C, T, HW, K) for B in (1, 3) for C in (1, 2, 3) for T in (1, 5, 17) for HW in (35, 385)
                for K in (1, 3, 8)] + [(3, 3, 5, 388, 3), (1, 2, 17, 388, 8)]
# accumulate / finish: the same axes, thinned to keep the test short (every value of every axis, both parities of C)
ACC_SHAPES = [(1, 1, 1, 35, 1), (3, 2, 5, 385, 3), (3, 3, 17, 35, 8), (1, 3, 5, 385, 8), (3, 1, 17, 385, 3),
              (2, 3, 5, 388, 4), (1, 2, 1, 35, 3)]
CONSTANT_VALUE = 17.25


def kernel_alpha(K):
    """nodes of the kernel tests: 0.0 first (the exact case), 1.0 last, irregular in between"""
    a = {1: [0.37], 3: [0.0, 0.37, 1.0]}.get(K)
    if a is None:
        a = [0.0] + list(_rng("alpha", K).uniform(0.0, 1.0, K - 2)) + [1.0]
    return np.asarray(a, dtype=F32)


def kernel_weights(K):
    return _rng("w", K).uniform(0.05, 0.6, K).astype(F32)


def stage_inputs(shape, kind):
    """(x [B,C,T,HW] fp32 in 0..255, base [B,C,T,HW] fp32 or None, value).  About a fifth of the elements have
    x == x0 exactly: with 'clip' copied from x, with 'constant' set to the value, with 'frozen' frame 0 copied into
    later frames (frame 0 itself always is)."""
    B, C, T, HW, K = shape
    g = _rng("stage", shape, kind)
    x = g.uniform(0.0, 255.0, (B, C, T, HW)).astype(F32)
    same = g.uniform(size=x.shape) < 0.2
    base = None
    if kind == CLIP:
        base = g.uniform(-40.0, 255.0, x.shape).astype(F32)
        base[same] = x[same]
    elif kind == CONSTANT:
        x[same] = F32(CONSTANT_VALUE)
    else:
        x = np.where(same, x[:, :, :1], x)
    return np.ascontiguousarray(x), base, CONSTANT_VALUE


def baseline(x, kind, base=None, value=0.0):
    """x0, same shape and dtype family as x ([B,C,T,...])"""
    if kind == FROZEN:
        return np.broadcast_to(x[:, :, :1], x.shape).copy()
    if kind == CONSTANT:
        return np.full_like(x, value)
    return np.asarray(base, dtype=x.dtype)


def windows(B, K):
    """(first, count) windows of the b*K rows: the whole list; one that starts mid-clip and, with three clips, crosses
    two clip boundaries; the last row alone"""
    total = B * K
    out = [(0, total)]
    first = K // 2
    last = 2 * K if B >= 3 else total - 1          # a row of clip 2
    if (first, last - first + 1) != out[0]:
        out.append((first, last - first + 1))
    if total > 1:
        out.append((total - 1, 1))
    return out


def stage_ref(x, x0, alpha):
    """[B,K,C,T,HW] float64: x0 + alpha (x - x0), alpha the fp32 node taken exactly"""
    x, x0 = x.astype(F64), x0.astype(F64)
    a = np.asarray(alpha, dtype=F32).astype(F64).reshape(1, -1, 1, 1, 1)
    return x0[:, None] + a * (x - x0)[:, None]


def stage_bound(x, x0):
    """[B,1,C,T,HW]: gamma(3) max(|x|, |x0|), for alpha in [0,1] (module docstring)"""
    return gamma(3) * np.maximum(np.abs(x.astype(F64)), np.abs(x0.astype(F64)))[:, None]


def to_layout(rows, layout, pad=np.nan):
    """rows [n,C,T,HW] -> the staged layout: NCTHW as is, or [n,T,HW,4] with the pad lanes set to `pad`"""
    if layout == 0:
        return np.ascontiguousarray(rows)
    n, C, T, HW = rows.shape
    out = np.full((n, T, HW, 4), pad, dtype=rows.dtype)
    out[..., :C] = rows.transpose(0, 2, 3, 1)
    return out


def from_layout(buf, layout, C):
    """the inverse: (rows [n,C,T,HW], pad lanes or None)"""
    if layout == 0:
        return buf, None
    return np.ascontiguousarray(buf[..., :C].transpose(0, 3, 1, 2)), buf[..., C:]


# ------------------------------------------------------------------------------------------------ accumulate / finish
def acc_inputs(shape):
    """(din [B,K,C,T,HW] fp32, w [K] fp32): gradients of both signs whose size differs by node and channel, so that a
    row read from the wrong node, clip or lane moves the sum"""
    B, C, T, HW, K = shape
    g = _rng("acc", shape)
    din = g.uniform(-1.0, 1.0, (B, K, C, T, HW)) * (1.0 + np.arange(K).reshape(1, K, 1, 1, 1)) \
        * (1.0 + 0.5 * np.arange(C).reshape(1, 1, C, 1, 1)) + 0.1 * np.arange(B).reshape(B, 1, 1, 1, 1)
    return din.astype(F32), kernel_weights(K)


def gsum_ref(din, w):
    """(Gsum [B,C,T,HW] float64, bound gamma(K + 1) sum_k |w_k g_k|)"""
    K = din.shape[1]
    t = din.astype(F64) * np.asarray(w, dtype=F32).astype(F64).reshape(1, K, 1, 1, 1)
    return t.sum(1), gamma(K + 1) * np.abs(t).sum(1)


def gsum_fp32(din, w):
    """the kernel's own arithmetic: fmaf per node, k ascending (float64 product and sum rounded once = fmaf exactly,
    since a product of two fp32 numbers is exact in float64 and the sum of it and an fp32 number rounds once to
    float64 -- double rounding aside, which the bit-exactness tests do not rest on)"""
    acc = np.zeros(din[:, 0].shape, dtype=F32)
    for k in range(din.shape[1]):
        acc = (din[:, k].astype(F64) * F64(w[k]) + acc.astype(F64)).astype(F32)
    return acc


def finish_ref(x, x0, gsum):
    """fp64 finish of fp32 (or fp64) inputs [B,C,T,HW]: dict of map, frames, abs_frames, total and their bounds"""
    B, C, T, HW = x.shape
    A = (x.astype(F64) - x0.astype(F64)) * gsum.astype(F64)
    absA = np.abs(A)
    out = {"A": A, "map": A.sum(1), "frames": A.sum((1, 3)), "abs_frames": absA.sum((1, 3)), "total": A.sum((1, 2, 3))}
    out["b_map"] = gamma(C + 1) * absA.sum(1)
    out["b_frames"] = gamma(C + HW) * absA.sum((1, 3))
    out["b_total"] = gamma(C + HW + T) * absA.sum((1, 2, 3))
    return out


def finish_inputs(shape, kind):
    """(x, base, value, Gsum fp32 [B,C,T,HW]) for the finish tests"""
    x, base, value = stage_inputs(shape, kind)
    din, w = acc_inputs(shape)
    return x, base, value, gsum_fp32(din, w)


# ------------------------------------------------------------------------------------------------ the whole of IG
def ig_pipeline(x, x0, alpha, w, grad_fn, dtype=F64):
    """IG in `dtype` (numpy): grad_fn(points [B*K,C,T,H,W] as `dtype`) -> (score [B*K], d score / d point).  Returns
    dict of map [B,T,H,W], frames, abs_frames [B,T], total [B], path_scores [B,K] (float64 arrays) and the points.

    mutant-free; the host test's mutants change the arguments or post-process."""
    B, C, T, H, W = x.shape
    K = len(alpha)
    x, x0 = x.astype(dtype), x0.astype(dtype)
    a = np.asarray(alpha, dtype=F32).astype(dtype).reshape(1, K, 1, 1, 1, 1)
    pts = (x0[:, None] + a * (x - x0)[:, None]).astype(dtype).reshape(B * K, C, T, H, W)
    score, g = grad_fn(pts)
    g = g.reshape(B, K, C, T, H, W).astype(dtype)
    gsum = np.zeros(x.shape, dtype=dtype)
    for k in range(K):
        gsum = (gsum + np.asarray(w[k], dtype=F32).astype(dtype) * g[:, k]).astype(dtype)
    A = ((x - x0) * gsum).astype(dtype)
    m = A.sum(1, dtype=dtype)
    fr = m.sum((2, 3), dtype=dtype)
    return {"map": m.astype(F64), "frames": fr.astype(F64), "abs_frames": np.abs(A).sum((1, 3, 4), dtype=dtype).astype(F64),
            "total": fr.sum(1, dtype=dtype).astype(F64), "path_scores": np.asarray(score, F64).reshape(B, K),
            "gsum": gsum.astype(F64), "points": pts}


# ------------------------------------------------------------------------------------------------ chain (ConvLSTM S2)
CHAIN_CASE = "S2"
CHAIN_K = 4
CHAIN_BASELINES = (("frozen", FROZEN, 0.0), ("constant", CONSTANT, 0.0))
# the first ids from the case's id0 on whose fp64 run has no ambiguous pool window at any of the K path points of
# either baseline (`python tests/ig_refs.py` prints them; test_ig_refs_host.py asserts it)
CHAIN_IDS = (200, 201)
CHAIN_TENSORS = ("map", "frames", "abs_frames", "total", "path_scores")


def chain_inputs(ids=None):
    case = CR.CASES[CHAIN_CASE]
    ids = CHAIN_IDS if ids is None else ids
    _, sd, _, _ = CR.case_inputs(case)
    x = CR.clips(case, ids)
    targets = [r % CR.K for r in range(len(ids))]
    return case, x, sd, targets


def _chain_grad_fn(case, sd, targets, K, dtype, keep=None):
    rowt = [t for t in targets for _ in range(K)]

    def fn(pts):
        res = CR.run(case, torch.from_numpy(np.ascontiguousarray(pts)), sd, dtype, targets=rowt)
        if keep is not None:
            keep.append(res)
        return res["score"], res["dx"]
    return fn


@functools.lru_cache(maxsize=None)
def chain_reference(baseline_name, ids=None):
    """Everything both tests need of the chain case under one baseline: inputs, the fp64 IG, the float32 floor and
    gate per tensor, and the ambiguous pool windows per path row."""
    case, x, sd, targets = chain_inputs(ids)
    kind, value = {n: (k, v) for n, k, v in CHAIN_BASELINES}[baseline_name]
    alpha, w = midpoint(CHAIN_K)
    x0 = baseline(x, kind, value=value)
    runs = []
    ref = ig_pipeline(x, x0, alpha, w, _chain_grad_fn(case, sd, targets, CHAIN_K, torch.float64, runs), F64)
    f32 = ig_pipeline(x, x0, alpha, w, _chain_grad_fn(case, sd, targets, CHAIN_K, torch.float32), F32)
    floor = OrderedDict((n, max(U, float(np.max(chain_err(f32[n], ref[n]))))) for n in CHAIN_TENSORS)
    # forward floors of the layers on the path rows themselves, for the ambiguity threshold
    pts = torch.from_numpy(ref["points"])
    fl, _ = CR.floors(case, pts, sd, runs[0], backward=False)
    amb, ties = CR.ambiguous_windows(runs[0]["pre"], fl)
    return {"case": case, "x": x, "x0": x0, "sd": sd, "targets": targets, "alpha": alpha, "w": w, "kind": kind,
            "value": value, "ref": ref, "f32": f32, "floor": floor,
            "gate": OrderedDict((n, CR.GATE_MARGIN * v) for n, v in floor.items()), "ambiguous": amb, "ties": ties}


def chain_err(a, r):
    """clstm_refs.elem_err per clip, on [b, ...] arrays"""
    r = np.asarray(r, F64)
    return CR.elem_err(np.asarray(a, F64).reshape(len(r), -1), r.reshape(len(r), -1))


MUTANTS = ("riemann", "nofactor", "prevframe", "dropchannel", "wtwice")


def chain_mutant(bundle, mutant):
    """fp64 IG of the chain case with one deliberate mistake (host test): left-Riemann nodes; the (x - x0) factor
    missing; the 'frozen' baseline taken from frame u-1 instead of frame 0; the last channel dropped from the sums;
    the weights applied twice."""
    case, x, sd, targets = bundle["case"], bundle["x"], bundle["sd"], bundle["targets"]
    alpha, w, x0 = bundle["alpha"], bundle["w"], bundle["x0"]
    if mutant == "riemann":
        alpha, w = left_riemann(CHAIN_K)
    if mutant == "wtwice":
        w = (w.astype(F64) ** 2).astype(F32)
    if mutant == "prevframe":
        x0 = np.concatenate([x[:, :, :1], x[:, :, :-1]], axis=2)
    out = ig_pipeline(x, x0, alpha, w, _chain_grad_fn(case, sd, targets, CHAIN_K, torch.float64), F64)
    if mutant in ("nofactor", "dropchannel"):
        A = out["gsum"] if mutant == "nofactor" else (x.astype(F64) - x0.astype(F64)) * out["gsum"]
        if mutant == "dropchannel":
            A = A[:, :-1]
        out["map"], out["frames"] = A.sum(1), A.sum((1, 3, 4))
        out["abs_frames"], out["total"] = np.abs(A).sum((1, 3, 4)), A.sum((1, 2, 3, 4))
    return out


def pick_chain_ids(n=2, limit=400):
    """the first n ids from the case's id0 on without an ambiguous window on any path row of either baseline"""
    case = CR.CASES[CHAIN_CASE]
    ids = []
    for i in range(case.id0, case.id0 + limit):
        ok = True
        for name, _, _ in CHAIN_BASELINES:
            b = chain_reference.__wrapped__(name, (i,))
            ok = ok and int(b["ambiguous"].sum()) == 0
        if ok:
            ids.append(i)
        if len(ids) == n:
            break
    return tuple(ids)


# ------------------------------------------------------------------------------------------------ I3D fixture gates
# tests/test_gpu_i3d.py:73-78, the whole-chain d(score)/d(input) gates: sampled L2, sampled max (relative to the largest
# reference entry); fp32-class arithmetic ("fp32", "bf16x6") and the 3-pass split
I3D_L2_GATE = {True: 3e-2, False: 5e-2}
I3D_MAX_GATE = {True: 4e-2, False: 1e-1}
I3D_EXACT = ("fp32", "bf16x6")
I3D_CLIPS = (21, 7)
I3D_BASELINES = (("frozen", "frozen", None), ("black", "constant", 0.0))      # fixture tag, engine baseline, base


if __name__ == "__main__":
    print("CHAIN_IDS =", pick_chain_ids())
