"""Case table, per-layer reference and gates for the TF-style ConvLSTM kernel tests (test_gpu_tfclstm_kernels.py on
the GPU, test_tfclstm_refs_host.py on the CPU).  Both iterate CASES, so the host test proves the reference, the
floors, the mutant distances and the zero-clip ambiguity cap on exactly the inputs the kernels are later compared on.

The reference is a functional torch-CPU restatement of oracle/tfclstm_ref.py (Keras ConvLSTM2D cell, MaxPooling2D
2x2 after every block, NHWC flatten, dense head, per-frame Grad-CAM) that runs in a given dtype and keeps, per
layer, the output sequence H[l], the pooled output X[l], through autograd dX[l] and dx, and the three recurrent-gate
pre-activations.  It runs in float64 (the reference proper) and in float32 (the floor: what a correct float32
implementation loses).  Nothing here needs a GPU or the HIP library.

Gate (DESIGN.md "TF-style ConvLSTM kernel gate"): per case and tensor, floor = elem_err(float32 run, float64 run),
the largest over the case's clips and never below U; a kernel tensor passes if every clip's elem_err against the
float64 run is at most GATE_MARGIN * floor.  The measure and the margins are those of clstm_refs.
"""
from collections import OrderedDict, namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from clstm_refs import GATE_MARGIN, TAU_MARGIN, U, ambiguous_windows, elem_err, pool2

K = 5                    # classes of every case
KINK = 2.5               # |z| at which hard_sigmoid's derivative jumps from 0.2 to 0

Case = namedtuple("Case", "id C T H W units kh kw s pad hard only_last b B xscale rscale tie forward_only wseed xseed")


def _case(id, C, T, H, W, units, k, s, pad, act, only_last, b, B, xscale=0.25, rscale=0.2, tie=False,
          forward_only=False, wseed=3, xseed=11):
    return Case(id, C, T, H, W, tuple(units), k[0], k[1], s, pad, act == "hard", only_last, b, B, xscale, rscale, tie,
                forward_only, wseed, xseed)


# The smallest shapes at which each branch of csrc/tf_clstm.hip exists.  wseed / xseed: seeds of the weights and of
# the clips: those of test_gpu_tfclstm.py wherever the float64 reference then has no ambiguous element of either kind
# (test_tfclstm_refs_host.py::test_zero_clip_cap).  G and S needed another xseed (pick_seeds below finds the first
# without an ambiguous element); theirs are from a wider scan that also kept the nearest element some tau away, since
# the floor, and tau with it, differs between CPUs (DESIGN.md "TF-style ConvLSTM kernel gate").
CASES = OrderedDict((c.id, c) for c in [
    # the geometry of test_gpu_tfclstm.py, now per layer
    _case("X", 1, 8, 30, 40, (4, 6), (3, 5), 2, "valid", "hard", True, 2, 2),
    # stride 1; odd 9 x 11 map: the pool drops a row and a column, the unpool writes zeros there; b < B
    _case("A", 2, 4, 9, 11, (3,), (3, 3), 1, "same", "hard", False, 3, 4),
    # even kernel: recurrent pads (0 front, 1 back) and (1, 2); odd x-pad on H; layer 1's kernel as wide as its map
    _case("B", 1, 5, 13, 18, (2, 3), (2, 4), 2, "same", "sigmoid", False, 2, 2),
    # stride 3, 'valid': input rows 18-19 and column 26 are never read, dx there is written and exactly 0
    _case("C", 2, 4, 20, 27, (5,), (3, 5), 3, "valid", "hard", False, 2, 2),
    # odd x-pad on W with stride 3, kernel larger than the stride
    _case("D", 1, 4, 16, 20, (3,), (5, 3), 3, "same", "sigmoid", True, 2, 2),
    # recurrent kernel 7 x 9 on a 4 x 5 map
    _case("E", 1, 3, 10, 13, (2,), (7, 9), 1, "valid", "hard", True, 2, 2),
    # T = 1: no t > 0 branch, no dC carry
    _case("F", 2, 1, 12, 16, (3, 2), (3, 3), 1, "same", "hard", True, 2, 2),
    # saturated gates in both layers
    _case("G", 1, 6, 30, 40, (4, 6), (3, 5), 2, "valid", "hard", False, 2, 2, xscale=0.75, rscale=0.6, xseed=50),
    # F = 1, three layers
    _case("H", 1, 4, 40, 48, (1, 5, 2), (3, 3), 1, "same", "sigmoid", False, 2, 2),
    # frames constant in space (values k/4, as case S8 of clstm_refs): exact pool ties, the first cell wins
    _case("S", 1, 3, 16, 24, (2,), (3, 3), 1, "same", "hard", False, 2, 2, tie=True, xseed=14),
    # 4.9 M work items: second grid-stride trip of tf_xconv_fwd_kernel.  Forward tensors and Grad-CAM only: at
    # 1.2 M pool windows the tau rule cannot hold (as P6 of the ConvLSTM table)
    _case("I", 1, 8, 120, 160, (8,), (3, 5), 1, "same", "hard", True, 4, 4, forward_only=True),
])

# Grad-CAM runs of the GPU test: (case, out_hw); None is the clip's own size.  Plane 99 with F = 3; a non-integer
# upscale of X's 3 x 3 plane; plane 19 200 with F = 8 (75 trips of the kernel's strided loops), down and up
CAM_RUNS = (("A", None), ("X", (45, 50)), ("I", (60, 80)), ("I", None))

MUTANTS = ("tap", "padfront", "nokink", "gateorder", "flatnchw", "poollast", "nodc", "clipmix")

# hard-sigmoid cases whose float64 run has a recurrent-gate pre-activation beyond the kink (asserted by
# test_tfclstm_refs_host.py::test_nokink_cases_are_the_saturated_ones)
NOKINK_CASES = ("X", "C", "E", "G")


def layer_dims(case):
    """[(Cin, F, Hin, Win, Ho, Wo, Hp, Wp)] by TensorFlow's rules ('valid': floor((n - k) / s) + 1, 'same': ceil(n / s))."""
    out, cin, H, W = [], case.C, case.H, case.W
    for Fu in case.units:
        if case.pad == "valid":
            Ho, Wo = (H - case.kh) // case.s + 1, (W - case.kw) // case.s + 1
        else:
            Ho, Wo = -(-H // case.s), -(-W // case.s)
        out.append((cin, Fu, H, W, Ho, Wo, Ho // 2, Wo // 2))
        cin, H, W = Fu, Ho // 2, Wo // 2
    return out


def mutant_applies(case, mutant):
    """tap and nodc need a recurrence (T >= 2); padfront an odd total 'same' pad (B, D: an odd kernel at stride 1
    pads symmetrically); nokink a saturated hard-sigmoid gate; flatnchw a top map on which the two flatten orders
    differ (F > 1 and more than one pooled cell: X and G pool their top layer to 1 x 1); poollast a constructed tie;
    clipmix a third clip."""
    if case.forward_only:
        return False
    _, Fu, _, _, _, _, Hp, Wp = layer_dims(case)[-1]
    return {"tap": case.T >= 2, "padfront": case.id in ("B", "D"), "nokink": case.id in NOKINK_CASES,
            "gateorder": True, "flatnchw": Fu > 1 and Hp * Wp > 1, "poollast": case.tie, "nodc": case.T >= 2,
            "clipmix": case.b >= 3 and case.T >= 2}[mutant]


# ------------------------------------------------------------------------------------------------ inputs
def fc_inputs(case):
    _, Fu, _, _, _, _, Hp, Wp = layer_dims(case)[-1]
    return Fu * Hp * Wp * (1 if case.only_last else case.T)


def case_inputs(case, b=None):
    """(x [b,C,T,H,W] float32, weights dict in Keras layouts (float32), targets [b]) of the case's first b clips."""
    b = case.b if b is None else b
    g = torch.Generator().manual_seed(case.wseed)
    layers, cin = [], case.C
    for Fu in case.units:
        layers.append((torch.randn(case.kh, case.kw, cin, 4 * Fu, generator=g) * case.xscale,
                       torch.randn(case.kh, case.kw, Fu, 4 * Fu, generator=g) * case.rscale,
                       torch.randn(4 * Fu, generator=g) * 0.1))
        cin = Fu
    w = dict(layers=layers, dense_w=torch.randn(fc_inputs(case), K, generator=g) * 0.2,
             dense_b=torch.randn(K, generator=g) * 0.1)
    if case.tie:
        x = torch.empty(case.B, case.C, case.T, case.H, case.W)
        for r in range(case.B):
            for t in range(case.T):
                x[r, :, t] = ((case.xseed + 3 * r + t) % 4 + 1) / 4.0
    else:
        x = torch.rand(case.B, case.C, case.T, case.H, case.W, generator=torch.Generator().manual_seed(case.xseed))
    return x[:b].contiguous(), w, [(r + 1) % K for r in range(b)]


# ------------------------------------------------------------------------------------------------ reference
def _pad_same(n, k, s, front_heavy=False):
    total = max((-(-n // s) - 1) * s + k - n, 0)
    lo = total // 2
    return (total - lo, lo) if front_heavy else (lo, total - lo)


def _conv(v, w_hwio, s, pad, front_heavy=False):
    """tf.nn.conv2d on NCHW v with a Keras HWIO kernel; 'same' pads by TensorFlow's rule, the odd cell at the back
    (front_heavy: at the front, mutant padfront)."""
    w = w_hwio.permute(3, 2, 0, 1)
    if pad == "same":
        pt, pb = _pad_same(v.shape[2], w.shape[2], s, front_heavy)
        pl, pr = _pad_same(v.shape[3], w.shape[3], s, front_heavy)
        v = F.pad(v, (pl, pr, pt, pb))
    return F.conv2d(v, w, stride=s)


def _rec_act(z, hard, nokink=False):
    if not hard:
        return torch.sigmoid(z)
    lin = 0.2 * z + 0.5
    y = torch.clamp(lin, 0.0, 1.0)
    return lin + (y - lin).detach() if nokink else y       # nokink: the value of the clamp, the slope 0.2 everywhere


def _flatten(X, only_last, nchw=False):
    """tf.layers.flatten of the NHWC maps of the last element or of the whole sequence (nchw: mutant flatnchw)."""
    b = X.shape[0]
    v = X if nchw else X.permute(0, 1, 3, 4, 2)
    return v[:, -1].reshape(b, -1) if only_last else v.reshape(b, -1)


def run(case, x, w, dtype=torch.float64, mutant=None, targets=None, backward=True):
    """The case's network on clips x in `dtype`.  Returns numpy float64 arrays: logits, probs [b,K]; per layer
    H[l] [b,T,F,Ho,Wo], X[l] [b,T,F,Hp,Wp] and z[l] [b,T,3,F,Ho,Wo] (pre-activations of the gates i, f, o); with
    backward also score [b], dX[l] and dx.  mutant: None or one of MUTANTS (a deliberately wrong network)."""
    T, s, hard = case.T, case.s, case.hard
    front = mutant == "padfront"
    layers = [tuple(t.to(dtype) for t in lw) for lw in w["layers"]]
    if mutant == "tap":                 # ONE recurrent weight of the top layer: [ky 0, kx 0, channel 0, output 0]
        k, rk, bias = layers[-1]
        rk = rk.clone()
        rk[0, 0, 0, 0] = 0
        layers[-1] = (k, rk, bias)
    b = x.shape[0]
    x = x.to(dtype).clone().requires_grad_(backward)
    v = x.permute(0, 2, 1, 3, 4)        # [b,T,C,H,W]
    Hs, Xs, Zs = [], [], []
    for (k, rk, bias) in layers:
        Fu = rk.shape[2]
        h = c = None
        outs, zs = [], []
        zx = _conv(v.reshape((b * T,) + tuple(v.shape[2:])), k, s, case.pad, front) + bias.view(1, -1, 1, 1)
        zx = zx.reshape((b, T) + tuple(zx.shape[1:]))               # the x-part of every step in one convolution
        for t in range(T):
            z = zx[:, t]
            if h is not None:
                hin = h[torch.arange(b) % 2] if mutant == "clipmix" else h
                z = z + _conv(hin, rk, 1, "same", front)
            if mutant == "gateorder":
                zi, zf, zo, zc = torch.split(z, Fu, dim=1)
            else:
                zi, zf, zc, zo = torch.split(z, Fu, dim=1)          # gate order i, f, c, o
            i, f, o = (_rec_act(q, hard, mutant == "nokink") for q in (zi, zf, zo))
            g = torch.tanh(zc)
            if c is None:
                c = i * g
            else:
                c = f * (c.detach() if mutant == "nodc" else c) + i * g
            h = o * torch.tanh(c)
            outs.append(h)
            zs.append(torch.stack([zi, zf, zo], 1).detach())
        out = torch.stack(outs, 1)
        pooled = pool2(out, last=(mutant == "poollast"))
        if backward:
            pooled.retain_grad()
        Hs.append(out)
        Xs.append(pooled)
        Zs.append(torch.stack(zs, 1))
        v = pooled
    flat = _flatten(Xs[-1], case.only_last, nchw=(mutant == "flatnchw"))
    logits = flat @ w["dense_w"].to(dtype) + w["dense_b"].to(dtype)
    probs = torch.softmax(logits, 1)

    def np64(t):
        return t.detach().to(torch.float64).numpy()
    res = {"logits": np64(logits), "probs": np64(probs), "H": [np64(t) for t in Hs], "X": [np64(t) for t in Xs],
           "z": [np64(t) for t in Zs]}
    if not backward:
        return res
    sc = probs[torch.arange(b), torch.as_tensor(targets)]
    res["score"] = np64(sc)
    sc.sum().backward()
    res["dX"] = [np64(t.grad) for t in Xs]
    res["dx"] = np64(x.grad)
    return res


def tensors(res, forward_only=False):
    """name -> [b, ...] array, in the order a fault is located: forward bottom-up, backward top-down."""
    o = OrderedDict()
    for l in range(len(res["X"])):
        o[f"H{l}"] = res["H"][l]
        o[f"X{l}"] = res["X"][l]
    o["logits"], o["probs"] = res["logits"], res["probs"]
    if forward_only or "dx" not in res:
        return o
    o["score"] = np.asarray(res["score"]).reshape(-1, 1)
    for l in reversed(range(len(res["dX"]))):
        o[f"dX{l}"] = res["dX"][l]
    o["dx"] = res["dx"]
    return o


def errors(res, ref, forward_only=False):
    """name -> per-clip elem_err of a run against the float64 reference."""
    tr, ta = tensors(ref, forward_only), tensors(res, forward_only)
    return OrderedDict((name, elem_err(ta[name], tr[name])) for name in tr)


def floors(case, x, w, ref, targets=None):
    """name -> max(U, elem_err(float32 run, float64 run)), the largest over the clips."""
    fo = case.forward_only
    r32 = run(case, x, w, torch.float32, targets=targets, backward=not fo)
    return OrderedDict((n, max(U, float(np.max(e)))) for n, e in errors(r32, ref, fo).items())


def kink_ambiguous(case, z, floor):
    """Per clip: (recurrent-gate pre-activations of the float64 run closer to the hard-sigmoid kink than
    TAU_MARGIN * floor(X[l]) * rms(z of that layer and clip), pre-activations beyond the kink).  A correct float32 run
    may put such an element on the other side, which changes its derivative from 0.2 to 0."""
    b = z[0].shape[0]
    amb, sat = np.zeros(b, np.int64), np.zeros(b, np.int64)
    if not case.hard:
        return amb, sat
    for l, v in enumerate(z):
        v = np.abs(v.reshape(b, -1))
        rms = np.sqrt(np.mean(v * v, axis=1, keepdims=True))
        amb += np.sum(np.abs(v - KINK) < TAU_MARGIN * floor[f"X{l}"] * rms, axis=1)
        sat += np.sum(v > KINK, axis=1)
    return amb, sat


def saturated_share(z):
    """Per layer: the share of recurrent-gate pre-activations with |z| > 2.5."""
    return [float(np.mean(np.abs(v) > KINK)) for v in z]


def reference(case, b=None):
    """Everything both tests need of a case on its first b clips: inputs, float64 run, floors, gates and the clips
    with an ambiguous element (the cap is zero: the host test asserts that there is none)."""
    x, w, targets = case_inputs(case, b)
    ref = run(case, x, w, torch.float64, targets=targets, backward=not case.forward_only)
    fl = floors(case, x, w, ref, targets)
    pool_amb, ties = ambiguous_windows(ref["H"], fl)
    kink_amb, sat = kink_ambiguous(case, ref["z"], fl)
    return {"x": x, "w": w, "targets": targets, "ref": ref, "floor": fl,
            "gate": OrderedDict((n, GATE_MARGIN * v) for n, v in fl.items()),
            "pool_ambiguous": pool_amb, "ties": ties, "kink_ambiguous": kink_amb, "saturated": sat,
            "left_out": [int(r) for r in np.nonzero(pool_amb + kink_amb)[0]]}


# ------------------------------------------------------------------------------------------------ Grad-CAM
def resize_bilinear(a, height, width):
    """Half-pixel bilinear resize with clamped source coordinates of the last two axes, in a's dtype (numpy)."""
    a = np.asarray(a)
    dt = a.dtype.type
    sh, sw = a.shape[-2:]
    ys = np.clip((np.arange(height, dtype=dt) + dt(0.5)) * (dt(sh) / dt(height)) - dt(0.5), 0, sh - 1).astype(dt)
    xs = np.clip((np.arange(width, dtype=dt) + dt(0.5)) * (dt(sw) / dt(width)) - dt(0.5), 0, sw - 1).astype(dt)
    y0, x0 = np.floor(ys).astype(np.int64), np.floor(xs).astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, sh - 1), np.minimum(x0 + 1, sw - 1)
    wy, wx = (ys - y0.astype(dt))[:, None], (xs - x0.astype(dt))[None, :]
    top = a[..., y0, :][..., x0] * (1 - wx) + a[..., y0, :][..., x1] * wx
    bot = a[..., y1, :][..., x0] * (1 - wx) + a[..., y1, :][..., x1] * wx
    return top * (1 - wy) + bot * wy


def gradcam(case, x, w, targets, dtype=torch.float64, out_hw=None):
    """Per-frame Grad-CAM of the unperturbed clips on the last block's output sequence, from the class LOGIT as the
    layers above see it (pool, flatten, dense; not through the recurrence), in `dtype`.  Returns {'frame', 'sequence':
    cam [b,T,oh,ow] (0/0 -> NaN), 'pre': the maps before the ReLU [b,T,Ho,Wo]}, float64 numpy."""
    res = run(case, x, w, dtype, backward=False)
    out = torch.from_numpy(res["H"][-1]).to(dtype).requires_grad_()
    flat = _flatten(pool2(out), case.only_last)
    logits = flat @ w["dense_w"].to(dtype) + w["dense_b"].to(dtype)
    b = out.shape[0]
    grad, = torch.autograd.grad(logits[torch.arange(b), torch.as_tensor(targets)].sum(), out)
    wts = grad.mean(dim=(3, 4), keepdim=True)                       # [b,T,F,1,1]
    pre = (wts * out.detach()).sum(2)                               # [b,T,Ho,Wo]
    cam = torch.clamp(pre, min=0).numpy()
    oh, ow = out_hw if out_hw is not None else (case.H, case.W)
    big = resize_bilinear(cam, oh, ow)
    fmax = cam.max(axis=(2, 3), keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"frame": (big / fmax).astype(np.float64),
                "sequence": (big / fmax.max(axis=1, keepdims=True)).astype(np.float64),
                "pre": pre.numpy().astype(np.float64)}


def cam_err(a, r):
    """elem_err of two maps with the same NaN pattern (the caller asserts that), NaN counted as 0."""
    return elem_err(np.nan_to_num(np.asarray(a, np.float64)), np.nan_to_num(r))


def gradcam_reference(case, out_hw=None, b=None):
    """float64 maps, the float32 floor and gate of each normalisation mode, and per clip the number of frames whose
    largest pre-ReLU value is non-zero but inside TAU_MARGIN * floor * rms(pre-ReLU maps of the clip): there a correct
    float32 run may turn a 0/0 frame into numbers or back."""
    x, w, targets = case_inputs(case, b)
    r64 = gradcam(case, x, w, targets, torch.float64, out_hw)
    r32 = gradcam(case, x, w, targets, torch.float32, out_hw)
    out = {"x": x, "w": w, "targets": targets, "ref": r64, "floor": {}, "gate": {}, "nan_equal": True}
    for mode in ("frame", "sequence"):
        out["nan_equal"] &= bool(np.array_equal(np.isnan(r32[mode]), np.isnan(r64[mode])))
        out["floor"][mode] = max(U, float(np.max(cam_err(r32[mode], r64[mode]))))
        out["gate"][mode] = GATE_MARGIN * out["floor"][mode]
    pre = r64["pre"]
    nb = pre.shape[0]
    top = np.abs(pre.max(axis=(2, 3)))                              # [b,T]
    rms = np.sqrt(np.mean(pre.reshape(nb, -1) ** 2, axis=1, keepdims=True))
    tau = TAU_MARGIN * max(out["floor"].values())
    out["ambiguous_frames"] = np.sum((top > 0) & (top < tau * rms), axis=1)
    return out


# ------------------------------------------------------------------------------------------------ seeds
def pick_seeds(case, tries=64):
    """The first (wseed, xseed) from the case's own on whose float64 run has no ambiguous pool window and no
    kink-ambiguous gate.  How the seeds of the table were made: `python tests/tfclstm_refs.py A B ...`."""
    for i in range(tries):
        cand = case._replace(xseed=case.xseed + i)
        bundle = reference(cand)
        if not bundle["left_out"]:
            return cand.wseed, cand.xseed
    raise RuntimeError(f"case {case.id}: no seed in {tries} tries")


if __name__ == "__main__":
    import sys
    for cid in sys.argv[1:]:
        print(cid, pick_seeds(CASES[cid]))
