"""Cases, per-op fp64 restatement, gates and mutants for the small-geometry I3D plan tests (test_gpu_i3d_small.py on
the GPU, test_i3d_refs_host.py on the CPU).  Both iterate the tables below.

What is restated is the WIRING of csrc/i3d_net.hip (build_plan, fill_conv_fwd / fill_conv_bwd / fill_pool,
launch_conv_site, run_forward / run_backward): which buffer and channel window every op reads and writes, which pads
and strides it is handed, which weights, scale and shift, and in which order the gradient of a buffer with several
writers is written, accumulated and gated.  Every op is one function of the numbers the kernels read:

  forward   want = relu(mode_sum(src window, w) * scale + shift), scale / shift the fp32 fold of bn_fold_kernel
            (scale = gamma / sqrtf(var + eps), shift = beta - mean * scale, unfused: the library is built with
            -ffp-contract=off); the fused [b0 | b1a | b2a] GEMM reads the three units' rows side by side
  backward  the transposed convolution of the downstream gradient with fl32(scale[co] * w) -- the product the backward
            packers round once -- cropped by the forward front pads, then base + v, then the ReLU gate `stored
            activation > 0` of the buffer written, applied by its LAST writer
  pools     the numpy rule of test_gpu_pool_blocks.py, bit for bit, dead-window marking where the plan sets it

`given`: the buffers each op reads.  The GPU test hands in the GPU's own buffers (so there are no gate flips and no
tie ambiguity, and nothing is left out); the host test hands in nothing and each op reads what the op before it gave,
through the storage rounding of the mode (the CHAIN), which in mode 'exact' (fp64 fold, no planes, no rounding) is the
reference network itself.

Error measure (conv_refs): |got - want| / A per element, A = sum |x||w| |scale| + |shift| (+ |base| where the buffer
has an earlier writer); floor = the same measure of a float32 CPU evaluation of the same op on the same inputs, never
below U; gate = GATE_MARGIN * floor; bf16 storage adds half a bf16 ulp of the stored value.  The floors are computed on
the chain's buffers on the CPU, per op, case and mode; nothing depends on a GPU measurement.
"""
from collections import OrderedDict, namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import ivf_arch as arch
import ivf_recipe as R
from clstm_refs import GATE_MARGIN
from conv_refs import (ACT_TERMS, MUTANT_DISTANCE, X3_TERMS, X6_TERMS, bf16_half_ulp, bf16_rne, conv_direct,  # noqa: F401
                       split_planes)
from leaf_refs import U, head_bwd_ref, head_fwd_ref, sum_bound  # noqa: F401
from test_gpu_pool_blocks import pool_bwd_ref, pool_fwd_ref

F64 = torch.float64
NUM_CLASSES = 6
MAX_BATCH = 3
CLIP_IDS = (3, 4, 5)
BN_EPS = 1e-3
SMOD = "Conv3d_1a_7x7,MaxPool3d_4a_3x3,MaxPool3d_5a_2x2"

Case = namedtuple("Case", "id clip engine modes")
CASES = OrderedDict((c.id, c) for c in [
    Case("odd", (3, 9, 33, 47), dict(head_hw=(2, 2)), ("fp32", "bf16x3", "bf16x6", "bf16act")),
    Case("smod", (3, 8, 33, 47), dict(stride_mod_layers=SMOD, last_stride=1, head_time_base=1, head_hw=(2, 2)),
         ("fp32", "bf16act")),
    Case("gray", (1, 5, 17, 31), dict(head_time_base=1, head_hw=(1, 1)), ("fp32", "bf16act")),
])
# the map sizes the issue's table states (stem, pool 2a, pool 3a, pool 4a, pool 5a): asserted by the host test
MAPS = {"odd": [(5, 17, 24), (5, 9, 12), (5, 5, 6), (3, 3, 3), (2, 2, 2)],
        "smod": [(8, 17, 24), (8, 9, 12), (8, 5, 6), (8, 3, 3), (8, 2, 2)],
        "gray": [(3, 9, 16), (3, 5, 8), (3, 3, 4), (2, 2, 2), (1, 1, 1)]}
CASE_MODES = [(c.id, m) for c in CASES.values() for m in c.modes]


def stride_mod(case):
    return case.engine.get("stride_mod_layers", ""), case.engine.get("last_stride", 1)


def head_window(case):
    sml, ls = stride_mod(case)
    return (arch.head_time_kernel(sml, ls, case.engine.get("head_time_base", 2)),) + tuple(case.engine["head_hw"])


def clips(case):
    return torch.from_numpy(np.stack([R.clip(i, *case.clip) for i in CLIP_IDS]))


def untied_clips(case):
    """The clips with a seeded fraction added to every pixel: no two pixels of a window are equal, so no pool window of
    the fp64 network has two distinct equal maxima (the host test counts them) and autograd routes as the rule does."""
    x = clips(case).double()
    g = torch.Generator().manual_seed(17)
    return x + torch.rand(x.shape, generator=g, dtype=F64) * 0.5


def state_dict(case):
    sml, ls = stride_mod(case)
    return R.i3d_state_dict(num_classes=NUM_CLASSES, in_channels=case.clip[0], stride_mod_layers=sml, last_stride=ls,
                            tag="i3d_kth")


def dout(case):
    g = torch.Generator().manual_seed(23)
    return (torch.randn(MAX_BATCH, NUM_CLASSES, generator=g) + 0.5).contiguous()


# ------------------------------------------------------------------------------------------------ the plan
Op = namedtuple("Op", "kind key src src_coff cin dst dst_coff cout k s pads units module dead dst2 n0")


def plan(case):
    """(bufs name -> (C, T, H, W, relu_out), ops in forward order) as build_plan lays them out."""
    C, T, H, W = case.clip
    sml, ls = stride_mod(case)
    bufs = OrderedDict(input=(4, T, H, W, False))
    ops = []

    def geom(src, k, s):
        dims = bufs[src][1:4]
        return tuple(arch.out_size(n, kk, ss) for n, kk, ss in zip(dims, k, s)), \
            tuple(arch.same_pad(n, kk, ss)[0] for n, kk, ss in zip(dims, k, s))

    def unit(name, src, cin, cout, k, s, src_coff=0, dst=None, dst_coff=0, module=None):
        outs, pads = geom(src, k, s)
        if dst is None:
            dst = name
            bufs[name] = (cout,) + outs + (True,)
        ops.append(Op("conv", name, src, src_coff, cin, dst, dst_coff, cout, k, s, pads, (name,), module, False, None, 0))
        return dst

    def pool(name, src, k, s, module=None):
        outs, pads = geom(src, k, s)
        bufs[name] = (bufs[src][0],) + outs + (False,)
        # a pool that is the sole writer of a ReLU output's gradient marks dead windows (fill_pool: o.bwd_mask)
        ops.append(Op("pool", name, src, 0, bufs[src][0], name, 0, bufs[src][0], k, s, pads, (), module,
                      module is None and bufs[src][4], None, 0))
        return name

    def ts(ep):
        return arch.temporal_stride(ep, sml, ls)

    x = unit("Conv3d_1a_7x7", "input", C, 64, (7, 7, 7), (ts("Conv3d_1a_7x7"), 2, 2))
    x = pool("MaxPool3d_2a_3x3", x, (1, 3, 3), (1, 2, 2))
    x = unit("Conv3d_2b_1x1", x, 64, 64, (1, 1, 1), (1, 1, 1))
    x = unit("Conv3d_2c_3x3", x, 64, 192, (3, 3, 3), (1, 1, 1))
    x = pool("MaxPool3d_3a_3x3", x, (1, 3, 3), (1, 2, 2))
    for m in arch.ENDPOINTS:
        if m == "MaxPool3d_4a_3x3":
            x = pool(m, x, (3, 3, 3), (ts(m), 2, 2))
        if m == "MaxPool3d_5a_2x2":
            x = pool(m, x, (2, 2, 2), (ts(m), 2, 2))
        if m not in arch.INCEPTION:
            continue
        cin, (c0, c1a, c1b, c2a, c2b, c3b) = arch.INCEPTION[m]
        assert bufs[x][0] == cin
        thw = bufs[x][1:4]
        bufs[m] = (c0 + c1b + c2b + c3b,) + thw + (True,)
        bufs[m + ".b12a"] = (c1a + c2a,) + thw + (True,)
        one = (1, 1, 1)
        ops.append(Op("group", m + ".grp", x, 0, cin, m, 0, c0 + c1a + c2a, one, one, (0, 0, 0),
                      (m + ".b0", m + ".b1a", m + ".b2a"), m, False, m + ".b12a", c0))
        unit(m + ".b1b", m + ".b12a", c1a, c1b, (3, 3, 3), one, 0, m, c0, m)
        unit(m + ".b2b", m + ".b12a", c2a, c2b, (3, 3, 3), one, c1a, m, c0 + c1b, m)
        pool(m + ".b3a", x, (3, 3, 3), one, m)
        unit(m + ".b3b", m + ".b3a", cin, c3b, one, one, 0, m, c0 + c1b + c2b, m)
        x = m
    return bufs, ops


def buffer_names(case):
    return list(plan(case)[0])


# ------------------------------------------------------------------------------------------------ weights
_W = {}


def weights(case, exact=False):
    """unit -> dict(w [cout,cin,k], scale, shift, wb = fl32(scale[co] * w)): float64 tensors holding the fp32 numbers
    the kernels multiply (exact: the fp64 fold of the fp64 state dict, i.e. the reference's BatchNorm); 'logits' has w
    [K, C] and bias."""
    key = (case.id, exact)
    if key in _W:
        return _W[key]
    sd = state_dict(case)
    out = {}
    for name, cin, cout, k, s, has_bn in arch.conv_units(case.clip[0], NUM_CLASSES, *stride_mod(case)):
        w = sd[name + ".conv3d.weight"]
        if not has_bn:
            out[name] = dict(w=torch.from_numpy(w.reshape(cout, cin)).double(),
                             bias=torch.from_numpy(sd[name + ".conv3d.bias"]).double())
            continue
        g, b, mu, var = (sd[f"{name}.bn.{q}"] for q in ("weight", "bias", "running_mean", "running_var"))
        if exact:
            g, b, mu, var, w = (v.astype(np.float64) for v in (g, b, mu, var, w))
            scale = g / np.sqrt(var + BN_EPS)
        else:
            scale = (g / np.sqrt(var + np.float32(BN_EPS))).astype(np.float32)
        shift = b - mu * scale
        wb = scale.reshape(-1, 1, 1, 1, 1) * w
        assert exact or (shift.dtype == np.float32 and wb.dtype == np.float32)
        out[name] = {q: torch.from_numpy(np.ascontiguousarray(v)).double()
                     for q, v in (("w", w), ("scale", scale), ("shift", shift), ("wb", wb))}
    _W[key] = out
    return out


# ------------------------------------------------------------------------------------------------ arithmetic modes
def operand_planes(mode, pixels=False):
    """(activation planes, weight planes, terms): conv_refs.operand_planes; pixels: the stem forward, which reads fp32
    pixels and in bf16act runs the 3-pass split."""
    if mode in ("fp32", "exact"):
        return 1, 1, ((0, 0),)
    if mode == "bf16x6":
        return 3, 3, X6_TERMS
    if mode == "bf16x3" or pixels:
        return 2, 2, X3_TERMS
    return 1, 2, ACT_TERMS


def mode_sum(mode, a, w, f, dtype=F64, pixels=False):
    """The mode's plane products through the bilinear map f, grouped by activation plane (f is linear in w, and the
    sums of weight planes are exact): sum_i f(a_i, sum_{j : (i, j) in TERMS} w_j)."""
    na, nw, terms = operand_planes(mode, pixels)
    ap, wp = split_planes(a, na), split_planes(w, nw)
    acc = None
    for i in range(na):
        if i > 0 and not bool(ap[i].any()):
            continue
        ws = sum(wp[j] for pi, j in terms if pi == i)
        t = f(ap[i].to(dtype), ws.to(dtype))
        acc = t if acc is None else acc + t
    return acc


def is16(mode, buf):
    return mode == "bf16act" and not buf.startswith("input")


def stored(mode, buf, t):
    """What the buffer holds of a computed value (the chain's storage rounding)."""
    if mode == "exact":
        return t
    return bf16_rne(t) if is16(mode, buf) else t.float().double()


# ------------------------------------------------------------------------------------------------ results
class Res:
    """One comparison: the window [c0, c1) of buffer `buf` (NCTHW).  kind 'A': per-element gate * A (+ bf16 slack);
    'bound': an explicit per-element bound (+ slack); 'exact': bit for bit."""
    def __init__(self, buf, c0, c1, want, A=None, bound=None, kind="A", raw=None):
        self.buf, self.c0, self.c1, self.want, self.A, self.bound, self.kind, self.raw = buf, c0, c1, want, A, bound, kind, raw


def slack(mode, res):
    return bf16_half_ulp(res.want) if is16(mode, res.buf) and res.kind != "exact" else torch.zeros_like(res.want)


def measure(got, res, mode):
    """max over elements of (|got - want| - slack)+ / A; 'bound' results: / bound; 'exact': 0 or inf."""
    d = (got.double() - res.want).abs()
    if res.kind == "exact":
        return 0.0 if bool((d == 0).all()) and not bool(torch.isnan(d).any()) else float("inf")
    d = torch.where(torch.isnan(d), d, (d - slack(mode, res)).clamp(min=0))
    den = res.A if res.kind == "A" else res.bound
    e = torch.where(d == 0, torch.zeros_like(d), d / den)
    return float(torch.nan_to_num(e, nan=float("inf"), posinf=float("inf")).max())


def ratio(got, res, mode, gate):
    """measured / gate: <= 1 passes ('bound' and 'exact' results carry their own bound: gate 1)."""
    m = measure(got, res, mode)
    return m / gate if res.kind == "A" else m


# ------------------------------------------------------------------------------------------------ the ops
def _shift_clips(t):
    return torch.cat([t[:1], t[:-1]], 0)


def conv_fwd(op, mode, Wd, a, dtype=F64, mutant=None):
    """a: the source window [b, cin, T, H, W] -> (want, A) [b, cout, To, Ho, Wo] of a Unit3D (conv, fold, ReLU)."""
    w = torch.cat([Wd[u]["w"] for u in op.units], 0)
    scale = torch.cat([Wd[u]["scale"] for u in op.units]).view(1, -1, 1, 1, 1)
    shift = torch.cat([Wd[u]["shift"] for u in op.units])
    if mutant == "grp_shift_own":          # b1a / b2a read the group's shift at their unit-relative column
        n = [Wd[u]["w"].shape[0] for u in op.units]
        shift = torch.cat([shift[:n[0]], shift[:n[1]], shift[:n[2]]])
    shift = shift.view(1, -1, 1, 1, 1)
    if a.shape[1] > w.shape[1]:
        w = F.pad(w, (0, 0, 0, 0, 0, 0, 0, a.shape[1] - w.shape[1]))
    pads = tuple(0 if (mutant == "conv_pad0") else p for p in op.pads)
    outs = tuple(arch.out_size(n, k, s) for n, k, s in zip(a.shape[2:], op.k, op.s))
    if mutant == "clip_shift":
        a = _shift_clips(a)

    def f(x, ww):
        return conv_direct(x, ww, op.s, pads, outs)
    v = mode_sum(mode, a, w, f, dtype, pixels=op.src == "input")
    want = torch.relu(v * scale.to(dtype) + shift.to(dtype))
    A = f(a.abs(), w.abs()) * scale.abs() + shift.abs()
    return want, A


def conv_bwd(op, mode, Wd, dy, in_thw, dtype=F64):
    """dy [b, cout(s), To, Ho, Wo] -> (v, A) [b, cin, T, H, W]: the ungated, unaccumulated backward-data of the op's
    units (a group: the fused GEMM over [dY_b0 | dT_b1a | dT_b2a])."""
    wb = torch.cat([Wd[u]["wb"] for u in op.units], 0)
    p = op.pads

    def f(g, ww):
        full = F.conv_transpose3d(g, ww, stride=op.s)
        return full[:, :, p[0]:p[0] + in_thw[0], p[1]:p[1] + in_thw[1], p[2]:p[2] + in_thw[2]]
    return mode_sum(mode, dy, wb, f, dtype), f(dy.abs(), wb.abs())


def _cl(t, np_dtype=np.float32):
    return np.ascontiguousarray(t.permute(0, 2, 3, 4, 1).numpy().astype(np_dtype))


def _nc(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 4, 1, 2, 3).double()


def _np_dtype(mode):
    return np.float64 if mode == "exact" else np.float32


def pool_fwd(op, x, dead=None, mutant=None, mode="fp32"):
    """x [b, C, T, H, W] (fp32-valued; mode 'exact': fp64) -> (y, code) by the numpy rule; code is channels-last uint8."""
    s, pads = op.s, op.pads
    outs = [arch.out_size(n, k, ss) for n, k, ss in zip(x.shape[2:], op.k, op.s)]
    if mutant == "pool_pad0":
        pads = (0, 0, 0)
    if mutant == "stride_t2":
        s = (2,) + tuple(op.s[1:])
        pads = (arch.same_pad(x.shape[2], op.k[0], 2)[0],) + tuple(pads[1:])
    dt = _np_dtype(mode)
    y, code = pool_fwd_ref(_cl(x, dt), op.k, s, list(pads), outs, op.dead if dead is None else dead, dt)
    return _nc(y), code


def pool_bwd(op, dy, code, x_shape, mode="fp32"):
    """dy [b, C, To, Ho, Wo] -> dX [b, C, T, H, W]: fp32 sums in ascending window order (bit for bit)."""
    b, C, T, H, W = x_shape
    dt = _np_dtype(mode)
    return _nc(pool_bwd_ref(_cl(dy, dt), code, (b, T, H, W, C), op.k, op.s, list(op.pads), None, None, dt))


# ------------------------------------------------------------------------------------------------ forward
def forward(case, mode, x, given=None, dtype=F64, mutant=None, ops_only=None):
    """x [b, C, T, H, W] fp32-valued.  Returns (results key -> Res in forward order, bufs name -> [b, C, T, H, W]).
    given None: the chain; else name -> the buffers the ops read.  mutant: (name, op key) -- one defect at one op.
    ops_only: evaluate these op keys alone (needs `given`)."""
    Wd = weights(case, mode == "exact")
    bufs_meta, ops = plan(case)
    b, C = x.shape[:2]
    res, cur = OrderedDict(), {}
    inp = torch.zeros((b, 4) + tuple(x.shape[2:]), dtype=F64)
    inp[:, :C] = x.double()
    cur["input"] = inp
    res["input"] = Res("input", 0, 4, inp, kind="exact")

    def src(name):
        return given[name] if given is not None else cur[name]

    def put(r):
        if r.buf not in cur:
            cur[r.buf] = torch.zeros((b,) + bufs_meta[r.buf][:4], dtype=F64)
        cur[r.buf][:, r.c0:r.c1] = stored(mode, r.buf, r.want) if r.kind != "exact" else r.want

    for op in ops:
        if ops_only is not None and op.key not in ops_only:
            continue
        mut = mutant[0] if mutant is not None and mutant[1] == op.key else None
        if op.kind == "pool":
            y, _ = pool_fwd(op, src(op.src), mutant=mut, mode=mode)
            out = [Res(op.dst, 0, op.cout, y, kind="exact")]
        else:
            coff = 0 if mut == "b2b_coff0" else op.src_coff
            a = src(op.src)[:, coff:coff + (4 if op.src == "input" else op.cin)]
            want, A = conv_fwd(op, mode, Wd, a, dtype, mut)
            if op.kind == "group":
                out = [Res(op.dst, 0, op.n0, want[:, :op.n0], A[:, :op.n0]),
                       Res(op.dst2, 0, op.cout - op.n0, want[:, op.n0:], A[:, op.n0:])]
            else:
                out = [Res(op.dst, op.dst_coff, op.dst_coff + op.cout, want, A)]
        for i, r in enumerate(out):
            res[op.key if i == 0 else op.dst2] = r
            put(r)
    if ops_only is None:
        feat = src("Mixed_5c")
        hk = head_window(case)
        assert tuple(feat.shape[2:]) == hk, (tuple(feat.shape[2:]), hk)
        fcl = feat.permute(0, 2, 3, 4, 1).reshape(b, -1, feat.shape[1])
        h = head_fwd_ref(fcl if dtype == F64 else fcl.float(), Wd["logits"]["w"], Wd["logits"]["bias"], True)
        res["logits"] = Res("logits", 0, NUM_CLASSES, h["logits"], bound=h["b_logits"], kind="bound")
        res["probs"] = Res("probs", 0, NUM_CLASSES, h["probs"], bound=1e-6 + 1e-5 * h["probs"], kind="bound")
        cur["logits"], cur["probs"] = h["logits"], stored("fp32" if mode != "exact" else mode, "probs", h["probs"])
    return res, cur


# ------------------------------------------------------------------------------------------------ backward
def backward(case, mode, acts, probs, target=None, dout=None, given=None, dtype=F64, mutant=None, cam=None,
             modules_only=None):
    """The gradient buffers top-down.  acts: name -> activation buffers (the ReLU gates, the pools' inputs); probs: the
    fp32 probabilities the head backward reads; given None: the chain, else name -> the `:grad` buffers the ops read
    (without the ':grad').  cam: the Grad-CAM target endpoint -- its gradient stays ungated, the pools it feeds keep true
    arg-max codes, and the walk stops there.  modules_only: evaluate the buffers of these Inception modules alone."""
    Wd = weights(case, mode == "exact")
    bufs_meta, ops = plan(case)
    b = probs.shape[0]
    res, cur = OrderedDict(), {}

    def g(name):
        return given[name] if given is not None else cur[name]

    def keep(key, r):
        res[key] = r
        if r.buf not in cur:
            cur[r.buf] = torch.zeros((b,) + bufs_meta[r.buf[:-5]][:4], dtype=F64)
        cur[r.buf[:-5]] = cur[r.buf]
        cur[r.buf][:, r.c0:r.c1] = stored(mode, r.buf[:-5], r.want) if r.kind != "exact" else r.want

    def gate_of(name):
        return (acts[name] > 0).double() if bufs_meta[name][4] and name != cam else None

    def mut(key):
        return mutant[0] if mutant is not None and mutant[1] == key else None

    if modules_only is None:
        feat = acts["Mixed_5c"]
        fcl = feat.permute(0, 2, 3, 4, 1).reshape(b, -1, feat.shape[1])
        h = head_bwd_ref(fcl, Wd["logits"]["w"], probs, target, dout, True, cam != "Mixed_5c")
        shp = (b,) + tuple(feat.shape[2:]) + (feat.shape[1],)
        keep("Mixed_5c:grad", Res("Mixed_5c:grad", 0, feat.shape[1], h["dfeat"].reshape(shp).permute(0, 4, 1, 2, 3),
                                  bound=h["b_dfeat"].reshape(shp).permute(0, 4, 1, 2, 3), kind="bound"))
    by_module = OrderedDict()
    for op in ops:
        by_module.setdefault(op.module or op.key, []).append(op)
    for name, mops in reversed(by_module.items()):
        if modules_only is not None and name not in modules_only:
            continue
        if cam is not None and name == cam:
            break
        if name in arch.INCEPTION:
            grp, b1b, b2b, p3, b3b = mops
            x, y, t12, t3 = grp.src, name, name + ".b12a", name + ".b3a"
            thw = bufs_meta[x][1:4]
            dY = g(y)
            # <m>.b3a:grad: b3b's transpose, ungated (a pool output)
            v, A = conv_bwd(b3b, mode, Wd, dY[:, b3b.dst_coff:b3b.dst_coff + b3b.cout], thw, dtype)
            keep(t3 + ":grad", Res(t3 + ":grad", 0, b3b.cin, v, A))
            # <m>.b12a:grad: two windows, each gated by .b12a > 0
            g12 = gate_of(t12)
            for u in (b2b, b1b):
                v, A = conv_bwd(u, mode, Wd, dY[:, u.dst_coff:u.dst_coff + u.cout], thw, dtype)
                gw = g12[:, u.src_coff:u.src_coff + u.cin]
                if mut(name) == "b12a_ungated":
                    gw = torch.ones_like(gw)
                keep(u.key + ":bwd", Res(t12 + ":grad", u.src_coff, u.src_coff + u.cin, v * gw.to(dtype), A))
            # module input: gate * (pool backward, written first + fused 1x1x1 GEMM, accumulated last)
            _, code = pool_fwd(p3, acts[x], dead=False, mode=mode)
            base = stored(mode, x, pool_bwd(p3, g(t3), code, acts[x].shape, mode))
            dcat = torch.cat([dY[:, :grp.n0], g(t12)], 1)
            v, A = conv_bwd(grp, mode, Wd, dcat, thw, dtype)
            gx = gate_of(x)
            gx = torch.ones_like(v, dtype=F64) if gx is None else gx
            m = mut(name)
            if m == "no_pool_branch":
                want = v * gx.to(dtype)
            elif m == "gate_first":
                want = base.to(dtype) * gx.to(dtype) + v
            else:
                want = (base.to(dtype) + v) * gx.to(dtype)
            keep(x + ":grad", Res(x + ":grad", 0, grp.cin, want, A + base.abs(), raw=base))
        elif mops[0].kind == "pool":
            op = mops[0]
            # sole writer: gated through the dead-window codes (not for the Grad-CAM target: true arg-max)
            _, code = pool_fwd(op, acts[op.src], dead=op.dead and op.src != cam, mode=mode)
            keep(op.src + ":grad", Res(op.src + ":grad", 0, op.cin,
                                       stored(mode, op.src, pool_bwd(op, g(op.dst), code, acts[op.src].shape, mode)), kind="exact"))
        else:
            op = mops[0]
            thw = bufs_meta[op.src][1:4]
            v, A = conv_bwd(op, mode, Wd, g(op.dst), thw, dtype)
            if op.src == "input":
                v, A = F.pad(v, (0, 0, 0, 0, 0, 0, 0, 4 - v.shape[1])), F.pad(A, (0, 0, 0, 0, 0, 0, 0, 4 - A.shape[1]), value=1.0)
            gs = gate_of(op.src)
            keep(op.src + ":grad", Res(op.src + ":grad", 0, v.shape[1], v if gs is None else v * gs.to(dtype), A))
    return res, cur


# ------------------------------------------------------------------------------------------------ chain, floors, gates
_REF = {}


def reference(case, mode):
    """The chain of a case in a mode on its three clips, both backward variants ('dout', 'target'), with the per-op
    floors and gates -- computed once and shared."""
    key = (case.id, mode)
    if key in _REF:
        return _REF[key]
    x = clips(case)
    fres, fbufs = forward(case, mode, x)
    f32, _ = forward(case, mode, x, given=fbufs, dtype=torch.float32)
    floor = OrderedDict()
    for k, r in fres.items():
        if r.kind == "A":
            floor[k] = max(U, measure(f32[k].want, r, "fp32"))
    probs = fbufs["probs"].float()
    target = probs.argmax(1).to(torch.int32)
    back = OrderedDict()
    for variant, kw in (("dout", dict(dout=dout(case))), ("target", dict(target=target))):
        bres, bbufs = backward(case, mode, fbufs, probs, **kw)
        b32, _ = backward(case, mode, fbufs, probs, given=bbufs, dtype=torch.float32, **kw)
        for k, r in bres.items():
            if r.kind == "A":
                floor[k] = max(U, floor.get(k, 0.0), measure(b32[k].want, r, "fp32"))
        back[variant] = (bres, bbufs)
    r = dict(x=x, fwd=fres, bufs=fbufs, probs=probs, target=target, back=back, floor=floor,
             gate=OrderedDict((k, GATE_MARGIN * v) for k, v in floor.items()))
    _REF[key] = r
    return r


def n_terms(case, key, mode):
    """Number of plane products in one output element of the op behind a floor key (+ scale, shift, base): what
    sum_bound bounds the floor with (conv_refs.n_terms)."""
    _, ops = plan(case)
    for op in ops:
        if op.kind == "pool":
            continue
        taps = op.k[0] * op.k[1] * op.k[2]
        fwd = taps * max(op.cin, 4) * len(operand_planes(mode, op.src == "input")[2])
        bwd = taps * op.cout * len(operand_planes(mode)[2])
        if key in (op.key, op.dst2):
            return fwd + 3
        if key == op.key + ":bwd" or (key == op.src + ":grad" and (op.kind == "group" or op.module is None)) or \
                (key == op.src + ":grad" and op.key.endswith(".b3b")):
            return bwd + 3
    raise KeyError(key)




# ------------------------------------------------------------------------------------------------ mutants
# name -> (case id, op key or module, direction): one wiring defect at one named site
MUTANTS = OrderedDict([
    ("b2b_coff0", ("gray", "Mixed_4c.b2b", "fwd")),            # b2b reads .b12a at channel 0
    ("b12_swapped", ("gray", "Mixed_4c", "fwd")),              # output windows of b1 and b2 in the other order
    ("no_pool_branch", ("gray", "Mixed_4c", "bwd")),           # pool branch dropped from the module-input gradient
    ("gate_first", ("gray", "Mixed_4c", "bwd")),               # gate before the last accumulation
    ("b12a_ungated", ("gray", "Mixed_4c", "bwd")),             # .b12a gradient left ungated
    ("pool_pad0", ("odd", "MaxPool3d_4a_3x3", "fwd")),         # front pad 0 where SAME gives 1
    ("conv_pad0", ("odd", "Mixed_3b.b1b", "fwd")),
    ("stride_t2", ("smod", "MaxPool3d_4a_3x3", "fwd")),        # temporal stride 2 at a stride-modified site
    ("head_count", ("odd", "head", "fwd")),                    # head mean over the wrong position count
    ("clip_shift", ("gray", "Mixed_4c.b1b", "fwd")),           # clip b reads clip b-1's buffer
    ("grp_shift_own", ("gray", "Mixed_4c.grp", "fwd")),        # fused group's BN shift from the unit's own offset
])


def mutant_distance(name, mode="fp32"):
    """How many gates the mutant's result sits from the restatement's, on the chain's buffers of its case: the largest
    over the buffers the site writes ('exact' results: inf when any element differs; the head: in bounds)."""
    cid, site, direction = MUTANTS[name]
    case = CASES[cid]
    ref = reference(case, mode)
    if name == "head_count":
        hk = head_window(case)
        feat = ref["bufs"]["Mixed_5c"]
        fcl = feat.permute(0, 2, 3, 4, 1).reshape(feat.shape[0], -1, feat.shape[1])
        h = head_fwd_ref(fcl * (fcl.shape[1] / (fcl.shape[1] + 1.0)), weights(case)["logits"]["w"],
                         weights(case)["logits"]["bias"], True)
        assert hk[0] * hk[1] * hk[2] == fcl.shape[1]
        return measure(h["logits"], ref["fwd"]["logits"], mode)
    if direction == "fwd":
        if name == "b12_swapped":
            m = site
            r1, r2 = ref["fwd"][m + ".b1b"], ref["fwd"][m + ".b2b"]
            want = torch.cat([r1.want, r2.want], 1)
            A = torch.cat([r1.A, r2.A], 1)
            gate = torch.cat([torch.full_like(r1.A, ref["gate"][m + ".b1b"]), torch.full_like(r2.A, ref["gate"][m + ".b2b"])], 1)
            swapped = torch.cat([r2.want, r1.want], 1)
            return float(((swapped - want).abs() / (gate * A)).max())
        res, _ = forward(case, mode, ref["x"], given=ref["bufs"], mutant=(name, site), ops_only=(site,))
        worst = 0.0
        for k, r in res.items():
            if k == "input":
                continue
            worst = max(worst, ratio(r.want, ref["fwd"][k], mode, ref["gate"].get(k, 1.0)))
        return worst
    bres, bbufs = ref["back"]["dout"]
    res, _ = backward(case, mode, ref["bufs"], ref["probs"], dout=dout(case), given=bbufs, mutant=(name, site),
                      modules_only=(site,))
    return max(ratio(r.want, bres[k], mode, ref["gate"].get(k, 1.0)) for k, r in res.items())


def pool_sites(case):
    return [op for op in plan(case)[1] if op.kind == "pool"]


def windows_with_ties(x, op):
    """Number of pool windows of x [b, C, T, H, W] whose POSITIVE maximum is held by two cells.  (A maximum of 0 -- ReLU
    zeros and pad cells -- routes to a cell whose own gate is shut, or to none: no gradient either way.)"""
    pads = [arch.same_pad(n, k, s) for n, k, s in zip(x.shape[2:], op.k, op.s)]
    xp = F.pad(x, (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1]))
    u = xp.unfold(2, op.k[0], op.s[0]).unfold(3, op.k[1], op.s[1]).unfold(4, op.k[2], op.s[2]).reshape(*xp.shape[:2], -1,
                                                                                                       op.k[0] * op.k[1] * op.k[2])
    top = u.topk(min(2, u.shape[-1]), dim=-1).values
    return int(((top[..., 0] == top[..., -1]) & (top[..., 0] > 0)).sum()) if u.shape[-1] > 1 else 0

