"""Case table, per-layer reference and gates for the ConvLSTM kernel tests (test_gpu_clstm_kernels.py on the GPU,
test_clstm_refs_host.py on the CPU).  Both iterate CASES, so the host test proves the reference, the floors, the
mutant distances and the pool-ambiguity cap on exactly the inputs the kernels are later compared on.

The reference is a functional torch-CPU restatement of the reference model (convolution_lstm.py:38-48 cell,
:96-132 unrolled stack with ONE shared BatchNorm2d and MaxPool2d(2); CLSTM_4.py:69-85 head), the same arithmetic as
oracle/clstm_ref.py but keeping every layer's pooled output X[l] (and, through autograd, its gradient dX[l]).  It
runs in float64 (the reference proper) and in float32 (the floor: what a correct float32 implementation loses).
Nothing here needs a GPU or the HIP library.

Gate (DESIGN.md "ConvLSTM kernel gate"): per case and tensor, floor = elem_err(float32 run, float64 run), the
largest over the case's clips; a kernel tensor passes if every clip's elem_err against the float64 run is at most
GATE_MARGIN * floor.
"""
from collections import OrderedDict, namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import ivf_recipe as R

U = 2.0 ** -24           # unit roundoff of float32
GATE_MARGIN = 8.0        # gate = GATE_MARGIN * floor
TAU_MARGIN = 32.0        # a pool window is ambiguous below TAU_MARGIN * (forward floor of the layer) * rms
AMBIGUOUS_CAP = 1.0 / 16  # at most this share of a P case's clips may be left out of the gradient comparisons
K = 5                    # classes of every case
SOLO_CLIP = 5            # the clip of a P case that is also run alone (b = 1, stepwise kernels)

Case = namedtuple("Case", "id path C T H W hid k s layers b B batch_norm softmax out_steps dout neg_bn tie id0")


def _case(id, path, C, T, H, W, hid, k, s, layers, b, B, batch_norm=True, softmax=True, out_steps=None, dout=False,
          neg_bn=False, tie=False, id0=None):
    return Case(id, path, C, T, H, W, hid, k, s, layers, b, B, batch_norm, softmax, out_steps, dout, neg_bn, tie, id0)


# path: 'S' stepwise split kernels (b < 64), 'P' persistent kernels (b = B = 64), 'W' wide kernels (hidden 8..32).
# id0: id of the case's first clip (clip r is id0 + r: every clip of a batch is distinct); chosen so that the
# float64 reference meets the ambiguity cap (test_clstm_refs_host.py::test_ambiguity_cap).
CASES = OrderedDict((c.id, c) for c in [
    # hidden 1; odd Ho (9 x 13) so the pool drops a row and the unpool must write zeros there; b < B
    _case("S1", "S", 1, 4, 18, 26, 1, 3, 1, 2, 3, 4, id0=100),
    # generic xconv_bwd with stride 2
    _case("S2", "S", 2, 6, 24, 32, 3, 3, 2, 2, 2, 2, id0=200),
    # xconv_bwd_k5s2<2> for both layers (2 input channels, hidden 2 feeding layer 1)
    _case("S3", "S", 2, 5, 24, 32, 2, 5, 2, 2, 2, 2, id0=300),
    # batch_norm = 0, softmax = 0, explicit dout, two output steps
    _case("S4", "S", 3, 3, 16, 24, 4, 5, 2, 1, 2, 2, batch_norm=False, softmax=False, out_steps=(0, 2), dout=True,
          id0=400),
    # k = MAXK on a 4 x 6 map (the kernel is larger than the map); three layers
    _case("S5", "S", 1, 5, 16, 24, 4, 7, 1, 3, 2, 2, id0=500),
    # T = 1: no t > 0 branch
    _case("S6", "S", 2, 1, 16, 24, 4, 5, 2, 2, 2, 2, id0=600),
    # S2 with a negative folded BN scale on channel 0: the pool must take its maximum AFTER the scale
    _case("S7", "S", 2, 6, 24, 32, 3, 3, 2, 2, 2, 2, neg_bn=True, id0=200),
    # constructed exact ties: frames constant in space (values k/4), so every interior 2 x 2 window ties exactly
    # and the first cell must win (pool mutant (c) is only visible here)
    _case("S8", "S", 1, 3, 16, 24, 2, 3, 1, 2, 3, 3, tie=True, id0=802),
    # planes 384 (exactly 6 waves) and 96 (128 threads: idle lanes in the last wave of layer 1)
    _case("P1", "P", 1, 5, 16, 24, 4, 5, 1, 2, 64, 64, id0=1100),
    # <1>; planes 96 and 6: fewer pixels than the 64 threads
    _case("P2", "P", 3, 4, 16, 24, 1, 3, 2, 2, 64, 64, id0=1200),
    # <3>
    _case("P3", "P", 2, 6, 24, 32, 3, 3, 2, 2, 64, 64, id0=1300),
    # <2> with k5s2<2>
    _case("P4", "P", 2, 5, 24, 32, 2, 5, 2, 2, 64, 64, id0=1400),
    # plane 5184 > 5 * 896 threads: second trip of the pixel-batch loop, partly live batches
    _case("P5", "P", 1, 3, 72, 72, 2, 5, 1, 1, 64, 64, id0=1500),
    # layer 0 needs 186 624 B of LDS and stays stepwise at b = 64; layer 1 is persistent
    _case("P6", "P", 1, 2, 104, 104, 4, 5, 1, 2, 64, 64, id0=1600),
    _case("W1", "W", 3, 4, 16, 24, 12, 3, 2, 2, 2, 2, id0=2100),
    _case("W2", "W", 1, 3, 12, 20, 20, 5, 1, 2, 2, 2, id0=2201),
    _case("W3", "W", 2, 3, 16, 16, 28, 3, 2, 2, 2, 2, id0=2300),
])

MUTANTS = ("tap", "cdelay", "poollast", "nodc", "clipmix")


def mutant_applies(case, mutant, b):
    """(a) tap and (b) cdelay need T >= 3, (c) poollast a constructed tie, (d) nodc a carry (T >= 2),
    (e) clipmix a third clip and a recurrence (T >= 2)."""
    return {"tap": case.T >= 3, "cdelay": case.T >= 3, "poollast": case.tie, "nodc": case.T >= 2,
            "clipmix": b >= 3 and case.T >= 2}[mutant]


# ------------------------------------------------------------------------------------------------ inputs
# Clip ids of the cases whose planes are so large that a run of consecutive ids breaks the ambiguity cap (a clip of
# P6 has 27 040 pool windows; at tau ~ 3e-5 about four of them are near-ties).  Chosen by pick_clip_ids below:
# the first ids from id0 on whose float64 run has no ambiguous window.  All ids of a case are distinct.
CLIP_IDS = {
    "P1": (
           1100, 1102, 1103, 1106, 1107, 1109, 1111, 1112, 1113, 1114, 1116, 1117, 1118, 1119, 1120, 1121,
           1122, 1123, 1124, 1125, 1126, 1127, 1130, 1132, 1134, 1135, 1136, 1138, 1140, 1141, 1142, 1143,
           1144, 1145, 1146, 1147, 1148, 1149, 1150, 1151, 1153, 1154, 1155, 1157, 1159, 1160, 1161, 1162,
           1163, 1164, 1167, 1168, 1169, 1170, 1171, 1172, 1173, 1174, 1176, 1177, 1178, 1179, 1182, 1183),
    "P5": (
           1501, 1502, 1503, 1505, 1506, 1507, 1508, 1509, 1510, 1515, 1516, 1517, 1518, 1519, 1520, 1521,
           1522, 1524, 1527, 1528, 1529, 1531, 1532, 1533, 1534, 1535, 1537, 1538, 1539, 1540, 1541, 1543,
           1545, 1546, 1547, 1548, 1549, 1551, 1554, 1557, 1558, 1560, 1563, 1565, 1567, 1568, 1569, 1571,
           1572, 1573, 1574, 1575, 1576, 1578, 1579, 1580, 1581, 1584, 1586, 1588, 1589, 1591, 1593, 1594),
    "P6": (
           1614, 1705, 1794, 1912, 1989, 2106, 2231, 2237, 2305, 2626, 2633, 2697, 2709, 2805, 2901, 2918,
           3026, 3236, 3307, 3416, 3423, 3447, 3701, 3862, 3926, 4055, 4078, 4136, 4304, 4348, 4368, 4380,
           4395, 4425, 4427, 4631, 4670, 4671, 4674, 4789, 4867, 4936, 4976, 5250, 5265, 5273, 5406, 5415,
           5502, 5623, 5689, 5697, 5860, 5917, 6021, 6088, 6150, 6187, 6229, 6255, 6415, 6429, 6467, 6498),
}


def clip_ids(case):
    return CLIP_IDS.get(case.id) or tuple(case.id0 + r for r in range(case.B))


def clips(case, ids):
    return (np.stack([R.clip(i, case.C, case.T, case.H, case.W) for i in ids]) / 255.0).astype(np.float32)


def case_inputs(case, b=None):
    """(x [b,C,T,H,W] float32, state dict of float32 tensors, targets [b], dout [b,K] or None) of the first b clips."""
    b = case.b if b is None else b
    C, T, H, W = case.C, case.T, case.H, case.W
    if case.tie:
        x = np.empty((b, C, T, H, W), np.float32)
        for r in range(b):
            for t in range(T):
                x[r, :, t] = ((case.id0 + 3 * r + t) % 4 + 1) / 4.0
    else:
        x = clips(case, clip_ids(case)[:b])
    n_out = len(case.out_steps) if case.out_steps else 1
    tag = "clstmk_S2" if case.id == "S7" else f"clstmk_{case.id}"
    sd = R.clstm_state_dict(num_classes=K, hidden=case.hid, channels=C, kernel=case.k, layers=case.layers,
                            image_size=(W, H), conv_stride=case.s, tag=tag, fc_mult=n_out)
    if case.neg_bn:
        sd["clstm.bn.weight"] = sd["clstm.bn.weight"].copy()
        sd["clstm.bn.weight"][0] *= -1.0
    sd = {k: v for k, v in R.to_torch(sd).items() if v.is_floating_point()}
    targets = [r % K for r in range(b)]
    dout = torch.from_numpy(R.uniform(f"clstmk_{case.id}/dout", (case.B, K), -1.0, 1.0))[:b] if case.dout else None
    return torch.from_numpy(x), sd, targets, dout


# ------------------------------------------------------------------------------------------------ reference
def pool2(v, last=False):
    """MaxPool2d(2) by hand: of the window's cells in the order (0,0) (0,1) (1,0) (1,1) the FIRST maximal one wins
    (last=True: the last one, mutant (c)); the gradient goes to that cell alone.  A trailing odd row / column is
    dropped."""
    Hp, Wp = v.shape[-2] // 2, v.shape[-1] // 2
    v = v[..., :2 * Hp, :2 * Wp]
    c = torch.stack([v[..., 0::2, 0::2], v[..., 0::2, 1::2], v[..., 1::2, 0::2], v[..., 1::2, 1::2]], -1)
    d = c.detach()
    w = torch.tensor([1, 2, 3, 4] if last else [4, 3, 2, 1])
    idx = ((d == d.amax(-1, keepdim=True)) * w).argmax(-1, keepdim=True)
    return c.gather(-1, idx).squeeze(-1)


def run(case, x, sd, dtype=torch.float64, fast_gates=False, mutant=None, targets=None, dout=None, backward=True):
    """The case's network on clips x in `dtype`.  Returns numpy float64 arrays: probs, logits [b,K]; X[l], pre[l]
    (post-BN, pre-pool) per layer as [b,T,hid,.,.]; with backward also score [b] (None with dout), dX[l] and dx.

    Upstream gradient: one-hot `targets` on the output (probs, or logits without softmax), or an explicit `dout`.
    fast_gates: tanh(v) = 2 sigmoid(2v) - 1 evaluated in `dtype` (the form of the persistent kernels).
    mutant: None, one of MUTANTS (a deliberately wrong network, for the host test), or 'nowh' (every Wh zeroed)."""
    L, hid, k, s, T = case.layers, case.hid, case.k, case.s, case.T
    sd = {key: v.to(dtype) for key, v in sd.items()}
    if mutant == "tap":                 # (a) one border tap of the top layer's Whf: ONE weight, [0, 0, ky 0, kx 0]
        w = sd[f"clstm.cell{L - 1}.Whf.weight"].clone()
        w[0, 0, 0, 0] = 0
        sd[f"clstm.cell{L - 1}.Whf.weight"] = w
    if mutant == "nowh":
        for key in list(sd):
            if ".Wh" in key:
                sd[key] = torch.zeros_like(sd[key])
    pad = (k - 1) // 2
    b = x.shape[0]
    x = x.to(dtype).clone().requires_grad_(backward)
    tanh = (lambda v: 2 * torch.sigmoid(2 * v) - 1) if fast_gates else torch.tanh
    state = [None] * L
    X = [[] for _ in range(L)]
    pre = [[] for _ in range(L)]
    for t in range(T):
        v = x[:, :, t]
        for l in range(L):
            p = f"clstm.cell{l}"
            if t == 0:
                z = v.new_zeros(b, hid, v.shape[2] // s, v.shape[3] // s)
                state[l] = (z, z.clone(), z.clone())
            h, c, c_old = state[l]
            if mutant == "clipmix":     # (e) clip r reads clip r % 2's hidden state
                h = h[torch.arange(b) % 2]
            cp = c_old if mutant == "cdelay" else c       # (b) c[t-1] read from t-2
            if mutant == "nodc":        # (d) the dC carry dropped
                cp = cp.detach()

            def gate(g):
                return (F.conv2d(v, sd[f"{p}.Wx{g}.weight"], sd[f"{p}.Wx{g}.bias"], s, pad)
                        + F.conv2d(h, sd[f"{p}.Wh{g}.weight"], None, 1, pad))
            ci = torch.sigmoid(gate("i"))
            cf = torch.sigmoid(gate("f"))
            cc = cf * cp + ci * tanh(gate("c"))
            co = torch.sigmoid(gate("o"))
            hn = co * tanh(cc)
            state[l] = (hn, cc, c)
            v = hn
            if case.batch_norm:
                v = F.batch_norm(v, sd["clstm.bn.running_mean"], sd["clstm.bn.running_var"], sd["clstm.bn.weight"],
                                 sd["clstm.bn.bias"], training=False, eps=1e-5)
            pre[l].append(v.detach())
            v = pool2(v, last=(mutant == "poollast"))
            if backward:
                v.retain_grad()
            X[l].append(v)
    steps = case.out_steps if case.out_steps else (T - 1,)
    flat = torch.cat([X[L - 1][e].reshape(b, -1) for e in steps], 1)     # per clip, in step order
    logits = F.linear(flat, sd["endFC.weight"], sd["endFC.bias"])
    probs = torch.softmax(logits, 1) if case.softmax else logits

    def np64(v):
        return v.detach().to(torch.float64).numpy()
    out = {"probs": np64(probs), "logits": np64(logits),
           "X": [np64(torch.stack(X[l], 1)) for l in range(L)],
           "pre": [np64(torch.stack(pre[l], 1)) for l in range(L)]}
    if not backward:
        return out
    if dout is not None:
        out["score"] = None
        (probs * dout.to(dtype)).sum().backward()
    else:
        sc = probs[torch.arange(b), torch.as_tensor(targets)]
        out["score"] = np64(sc)
        sc.sum().backward()
    out["dX"] = [np64(torch.stack([v.grad if v.grad is not None else torch.zeros_like(v) for v in X[l]], 1))
                 for l in range(L)]
    out["dx"] = np64(x.grad)
    return out


def tensors(res, forward_only=False):
    """name -> [b, ...] array, in the order a fault is located: forward bottom-up, backward top-down."""
    o = OrderedDict()
    for l, v in enumerate(res["X"]):
        o[f"X{l}"] = v
    o["logits"], o["probs"] = res["logits"], res["probs"]
    if forward_only or "dx" not in res:
        return o
    if res.get("score") is not None:
        o["score"] = np.asarray(res["score"]).reshape(-1, 1)
    for l in reversed(range(len(res["dX"]))):
        o[f"dX{l}"] = res["dX"][l]
    o["dx"] = res["dx"]
    return o


GRADIENT_TENSORS = ("score", "dX", "dx")      # prefixes of what an ambiguous clip is left out of


def is_gradient(name):
    return name.startswith(GRADIENT_TENSORS)


# ------------------------------------------------------------------------------------------------ measures
def elem_err(a, r):
    """Per clip (leading axis): max over elements of |a - r| / (|r| + rms(r)), rms over the clip's own tensor.  One
    wrong element is measured against the tensor's typical size, never against its maximum.  NaN in `a` gives NaN."""
    a = np.asarray(a, np.float64).reshape(len(r), -1)
    r = np.asarray(r, np.float64).reshape(len(r), -1)
    d = np.abs(a - r)
    den = np.abs(r) + np.sqrt(np.mean(r * r, axis=1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(d == 0, 0.0, d / den)
    return np.max(e, axis=1)


def errors(res, ref, forward_only=False):
    """name -> per-clip elem_err of a run against the float64 reference."""
    tr = tensors(ref, forward_only)
    ta = tensors(res, forward_only)
    return OrderedDict((name, elem_err(ta[name], tr[name])) for name in tr)


def floors(case, x, sd, ref, targets=None, dout=None, backward=True):
    """name -> floor of the case: elem_err(float32 run, float64 run), the largest over the clips, with libm gates,
    and for the P cases the larger of libm and fast_gates (the persistent kernels evaluate tanh that way).  Never
    below one float32 rounding.  Also returns the per-variant figures for the record."""
    variants = OrderedDict()
    for name, fast in (("libm", False),) + ((("fast", True),) if case.path == "P" else ()):
        r32 = run(case, x, sd, torch.float32, fast_gates=fast, targets=targets, dout=dout, backward=backward)
        variants[name] = OrderedDict((n, float(np.max(e))) for n, e in errors(r32, ref, not backward).items())
    fl = OrderedDict((n, max(U, max(v[n] for v in variants.values()))) for n in variants["libm"])
    return fl, variants


def ambiguous_windows(pre, forward_floor):
    """Per clip: (number of 2 x 2 pool windows whose two largest post-BN values differ by less than tau * rms in
    the float64 run, number of exactly tied windows).  tau = TAU_MARGIN * the layer's forward floor; rms over the
    clip's post-BN tensor of that layer.  Such a window can route the gradient to another cell in float32 without
    any bug.  An exact float64 tie is structural (equal inputs through equal arithmetic, case S8), stays tied in
    float32, and is decided by the first-cell rule: it is counted apart and is not ambiguous."""
    b = pre[0].shape[0]
    amb = np.zeros(b, np.int64)
    ties = np.zeros(b, np.int64)
    for l, v in enumerate(pre):
        Hp, Wp = v.shape[-2] // 2, v.shape[-1] // 2
        v = v[..., :2 * Hp, :2 * Wp]
        c = np.stack([v[..., 0::2, 0::2], v[..., 0::2, 1::2], v[..., 1::2, 0::2], v[..., 1::2, 1::2]], -1)
        c = np.sort(c, -1)
        gap = (c[..., 3] - c[..., 2]).reshape(b, -1)
        rms = np.sqrt(np.mean(pre[l].reshape(b, -1) ** 2, axis=1, keepdims=True))
        tau = TAU_MARGIN * forward_floor[f"X{l}"]
        amb += np.sum((gap > 0) & (gap < tau * rms), axis=1)
        ties += np.sum(gap == 0, axis=1)
    return amb, ties


def reference(case, b=None):
    """Everything both tests need of a case on its first b clips: inputs, float64 run, floors, gates, and the clips
    left out of the gradient comparisons."""
    x, sd, targets, dout = case_inputs(case, b)
    ref = run(case, x, sd, torch.float64, targets=targets, dout=dout)
    fl, variants = floors(case, x, sd, ref, targets, dout)
    amb, ties = ambiguous_windows(ref["pre"], fl)
    return {"x": x, "sd": sd, "targets": targets, "dout": dout, "ref": ref, "floor": fl, "variants": variants,
            "gate": OrderedDict((n, GATE_MARGIN * v) for n, v in fl.items()), "ambiguous": amb, "ties": ties,
            "left_out": [int(r) for r in np.nonzero(amb)[0]]}


def pick_clip_ids(case, n=None, chunk=64):
    """The first n ids from case.id0 on whose clip has no ambiguous window, with tau from the forward floors of the
    case's current clips.  How the CLIP_IDS entries were made: `python tests/clstm_refs.py P6`."""
    n = case.B if n is None else n
    x, sd, _, _ = case_inputs(case)
    fl, _ = floors(case, x, sd, run(case, x, sd, torch.float64, backward=False), backward=False)
    ids, nxt = [], case.id0
    while len(ids) < n:
        cand = list(range(nxt, nxt + chunk))
        nxt += chunk
        ref = run(case, torch.from_numpy(clips(case, cand)), sd, torch.float64, backward=False)
        amb, _ = ambiguous_windows(ref["pre"], fl)
        ids += [i for i, a in zip(cand, amb) if a == 0]
    return tuple(ids[:n])


if __name__ == "__main__":
    import sys
    for cid in sys.argv[1:]:
        print(f'    "{cid}": {pick_clip_ids(CASES[cid])},')
