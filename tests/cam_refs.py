"""fp64 restatement of the Grad-CAM family (csrc/cam_ops.hip), its forward-error gate and the synthetic
cases of the kernel tests.  numpy only.

Definitions, per clip, A and G [npos, C] (p = position, k = channel), s_k = sum_p A[p,k]:

    gradcam     w_k = (sum_p G) / npos                       cam[p] = relu(sum_k w_k A[p,k])
    gradcam++   w_k = sum_p [G > 0] G / (2 + s_k G)          cam[p] = relu(sum_k w_k A[p,k])
    xgradcam    w_k = (sum_p G A) / s_k, 0 where s_k == 0    cam[p] = relu(sum_k w_k A[p,k])
    hirescam    w_k = 0                                      cam[p] = relu(sum_k G[p,k] A[p,k])
    layercam    w_k = 0                                      cam[p] = relu(sum_k relu(G[p,k]) A[p,k])

The gate (`bounds`) is a forward-error bound of an fp32 evaluation in ANY summation order, evaluated in fp64 per
output element; u = 2^-24 is the unit round-off of fp32 and every bound below is first order in u with the second
order covered by the "+2".

  * A sum of n fp32 products: each product is rounded once and takes part in at most n - 1 additions, so
    |err| <= (n + 2) u sum|terms|.  This bounds s_k (n = npos, the "products" are A itself), sum_p G, sum_p G A and
    the map sums over k (n = C).  Inputs are exact: the synthetic values are bf16-representable, so both storages
    load the same numbers.
  * gradcam: w = S / npos adds the rounding of the division and of float(npos): dw = dS / npos + 2 u |w|.
  * xgradcam: w = N / s with N = sum G A:  dw = (dN + |w| ds) / (|s| - ds) + 4 u |w|  (quotient rule with the
    perturbed denominator kept, the division and the two fp64 -> fp32 conversions of the ConvLSTM kernel).  Where
    s_k == 0 exactly the weight is 0 with bound 0 (the cases keep |s_k| >= 1e-3 sum|A| otherwise, see `preconditions`).
  * gradcam++: a term is t = G / d, d = 2 + s G, computed as fl(fl(1 / fl(2 + fl(s G))) G): four roundings, the first
    one scaled by |s G| / |d| on its way through the sum, so the term's own error is u (4 + |s G / d|) |t|.  The error
    of s enters through alpha = 1 / (2 + s G): |d alpha / d s| = G / d^2; by the mean value theorem over [s - ds, s + ds],
    where the denominator stays above |d| - G ds in magnitude, dt <= G^2 ds / (|d| (|d| - G ds))  (|d| > 2 G ds is
    asserted).  Then dw = (n + 2) u sum|t| + sum dt.
  * maps of the weighted kinds: |err| <= (C + 2) u sum_k |w_k A| + sum_k dw_k |A[p,k]|; of hirescam and layercam:
    (C + 2) u sum_k |G A| resp. sum_k relu(G) |A|.  The final ReLU is 1-Lipschitz and keeps the bound.

`bounds` never looks at the values under test.  The mutants of `family(..., mutant=)` show the gate is not vacuous
(test_cam_refs_host.py)."""
import numpy as np

KINDS = ("gradcam", "gradcam++", "xgradcam", "hirescam", "layercam")
KIND_ID = {k: i for i, k in enumerate(KINDS)}
WEIGHTED = KINDS[:3]
U = 2.0 ** -24
MUTANTS = ("pp_no_relu", "layer_no_relu", "s_one_short", "xgrad_mean", "pp_const_1", "map_drops_last_channel")


def bf16_round(x):
    """nearest-even rounding of fp32 to the bf16 grid, returned as fp32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def to_bf16_bits(x):
    """uint16 storage of bf16-exact fp32 values"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    assert not np.any(u & np.uint32(0xFFFF)), "values are not bf16-representable"
    return (u >> np.uint32(16)).astype(np.uint16)


def _map_sum(W, A, mutant):
    if mutant == "map_drops_last_channel":
        return (W[..., :-1] * A[:, :-1]).sum(axis=1)
    return (W * A).sum(axis=1)


def family(A, G, kinds=KINDS, mutant=None, dtype=np.float64):
    """A, G [npos, C] -> {kind: dict(w [C], pre [npos] before the ReLU, cam [npos])}.  With divide-by-zero the
    non-finite values propagate as numpy gives them."""
    A = np.asarray(A, dtype=dtype)
    G = np.asarray(G, dtype=dtype)
    npos, C = A.shape
    s = (A[:-1] if mutant == "s_one_short" else A).sum(axis=0)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for kind in kinds:
            if kind == "gradcam":
                w = G.sum(axis=0) / dtype(npos)
                pre = _map_sum(w[None], A, mutant)
            elif kind == "gradcam++":
                two = dtype(1 if mutant == "pp_const_1" else 2)
                d = two + s[None] * G
                t = G / d
                if mutant != "pp_no_relu":
                    t = np.where(G > 0, t, 0)
                w = t.sum(axis=0)
                pre = _map_sum(w[None], A, mutant)
            elif kind == "xgradcam":
                num = (G * A).mean(axis=0) if mutant == "xgrad_mean" else (G * A).sum(axis=0)
                w = np.where(s == 0, 0, num / np.where(s == 0, 1, s))
                pre = _map_sum(w[None], A, mutant)
            elif kind == "hirescam":
                w = np.zeros(C, dtype)
                pre = _map_sum(G, A, mutant)
            elif kind == "layercam":
                w = np.zeros(C, dtype)
                pre = _map_sum(G if mutant == "layer_no_relu" else np.maximum(G, 0), A, mutant)
            else:
                raise ValueError(kind)
            out[kind] = dict(w=w, pre=pre, cam=np.maximum(pre, 0))
    return out


def family32(A, G, order):
    """The same in fp32, two summation orders: 'pairwise' (np.sum) and 'reversed' (a sequential loop from the last
    term to the first, np.add.accumulate on the flipped axis)."""
    A = np.asarray(A, np.float32)
    G = np.asarray(G, np.float32)

    def red(x, axis):
        if order == "pairwise":
            return x.sum(axis=axis, dtype=np.float32)
        return np.take(np.add.accumulate(np.flip(x, axis), axis=axis, dtype=np.float32), -1, axis=axis)
    npos, C = A.shape
    s = red(A, 0)
    out = {}
    w = red(G, 0) / np.float32(npos)
    out["gradcam"] = (w, red(w[None] * A, 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(G > 0, (np.float32(1) / (np.float32(2) + s[None] * G)) * G, np.float32(0))
    w = red(t, 0)
    out["gradcam++"] = (w, red(w[None] * A, 1))
    w = np.where(s == 0, np.float32(0), red(G * A, 0) / np.where(s == 0, np.float32(1), s))
    out["xgradcam"] = (w, red(w[None] * A, 1))
    z = np.zeros(C, np.float32)
    out["hirescam"] = (z, red(G * A, 1))
    out["layercam"] = (z, red(np.maximum(G, 0) * A, 1))
    return {k: dict(w=w, pre=p, cam=np.maximum(p, 0)) for k, (w, p) in out.items()}


def bounds(A, G, kinds=KINDS, singular="raise"):
    """{kind: dict(w [C], cam [npos])}: the gate of the module docstring, fp64.  Where a Grad-CAM++ denominator can
    reach 0 inside the error of s_k (|d| <= 2 G ds: possible on signed maps only) no forward bound exists: that is an
    error, or with singular="inf" the bound of that channel's weight, and of every map value it enters, is infinite."""
    A = np.asarray(A, np.float64)
    G = np.asarray(G, np.float64)
    npos, C = A.shape
    aA = np.abs(A)
    s = A.sum(axis=0)
    ds = (npos + 2) * U * aA.sum(axis=0)
    out = {}
    for kind in kinds:
        if kind == "gradcam":
            w = G.sum(axis=0) / npos
            dw = (npos + 2) * U * np.abs(G).sum(axis=0) / npos + 2 * U * np.abs(w)
        elif kind == "gradcam++":
            pos = G > 0
            d = np.where(pos, 2 + s[None] * G, 1.0)
            t = np.where(pos, G / d, 0.0)
            gds = np.where(pos, G * ds[None], 0.0)
            ok = np.abs(d) > 2 * gds
            assert singular == "inf" or ok.all(), "the Grad-CAM++ denominator is too close to 0 for a bound"
            safe = np.where(ok, np.abs(d) * (np.abs(d) - gds), 1.0)
            dt = U * (4 + np.abs(s[None] * G / d)) * np.abs(t) + np.where(ok, np.where(pos, G * gds, 0.0) / safe, np.inf)
            w = t.sum(axis=0)
            dw = (npos + 2) * U * np.abs(t).sum(axis=0) + dt.sum(axis=0)
        elif kind == "xgradcam":
            num = (G * A).sum(axis=0)
            dnum = (npos + 2) * U * np.abs(G * A).sum(axis=0)
            nz = s != 0
            sd = np.where(nz, s, 1.0)
            w = np.where(nz, num / sd, 0.0)
            assert np.all(np.abs(sd) > 2 * ds * nz), "s_k too close to 0 for a bound"
            dw = np.where(nz, (dnum + np.abs(w) * ds) / (np.abs(sd) - ds * nz) + 4 * U * np.abs(w), 0.0)
        if kind in WEIGHTED:
            dcam = (C + 2) * U * (np.abs(w)[None] * aA).sum(axis=1) + np.where(aA > 0, dw[None] * aA, 0.0).sum(axis=1)
        elif kind == "hirescam":
            dw = np.zeros(C)
            dcam = (C + 2) * U * (np.abs(G) * aA).sum(axis=1)
        elif kind == "layercam":
            dw = np.zeros(C)
            dcam = (C + 2) * U * (np.maximum(G, 0) * aA).sum(axis=1)
        out[kind] = dict(w=dw, cam=dcam)
    return out


def excess(got, ref, bound):
    """max over elements of |got - ref| / bound (0 / 0 = 0): <= 1 passes the gate"""
    diff = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    bound = np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, 0.0, diff / bound)
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------ layouts
def clstm_positions(X, steps):
    """[T, hid, plane] (or [T, hid, Hp, Wp]) of one clip -> [n_steps * plane, hid], positions ordered (step, pixel)"""
    X = np.asarray(X)[list(steps)]
    X = X.reshape(X.shape[0], X.shape[1], -1)
    return X.transpose(0, 2, 1).reshape(-1, X.shape[1])


# ------------------------------------------------------------------ synthetic cases
def synth(B, npos, C, seed, signed=False):
    """A, G [B, npos, C] fp32 with bf16-representable values:
      * A >= 0 (or of mixed sign with `signed`, the ConvLSTM's post-BN maps), one all-zero channel (index 1, C >= 4);
      * G of mixed sign, scaled per channel so that s_k G spans about -1.5 .. 8 (-0.95 .. 8 with `signed`, where a
        positive G can sit on a negative s_k and the Grad-CAM++ denominator 2 + s_k G must stay >= 1);
      * one channel whose G is <= 0 everywhere (index 2, C >= 4);
      * a per-position and a per-channel component in G, so that the weights and the HiResCAM sums change sign."""
    rng = np.random.default_rng(seed)
    o = rng.normal(0, 0.5 if signed else 1.0, (B, 1, C))      # per-channel component of G: the sign of the weight
    if signed:
        A = rng.normal(0.15, 1.0, (B, npos, C))
    else:
        # post-ReLU: zeros, and a position fires mostly the channels of one weight sign, or a sum of w_k A[p,k] over
        # many channels with A >= 0 would never change sign
        tau = np.where(rng.uniform(0, 1, (B, npos, 1)) < 0.5, 1.0, -1.0)
        fire = np.where(np.sign(o) == tau, 0.85, 0.2)
        A = rng.uniform(0.0, 2.0, (B, npos, C)) * (rng.uniform(0, 1, (B, npos, C)) < fire)
    A = bf16_round(A.astype(np.float32)).astype(np.float64)
    if signed:      # keep |s_k| >= 5 % of sum|A|: move the channel's first entry (re-rounded; the tests re-check)
        for _ in range(4):
            s, sa = A.sum(axis=1), np.abs(A).sum(axis=1)
            fix = np.abs(s) < 0.05 * sa
            A[:, 0, :] = bf16_round((A[:, 0, :] + fix * 0.2 * sa).astype(np.float32))
    if C >= 4:
        A[:, :, 1] = 0.0
    s = A.sum(axis=1)                                                  # exact: fp64 sum of bf16 values
    z = rng.normal(0, 1.2, (B, npos, 1))
    e = rng.normal(-0.45, 0.5, (B, npos, C)) + (rng.uniform(0, 1, (B, npos, C)) < 0.1) * rng.uniform(2, 7, (B, npos, C))
    g = np.clip(z + o + e, -0.95 if signed else -1.5, 8.0)
    G = g / np.where(s == 0, 1.0, s)[:, None, :]
    if C >= 4:
        G[:, :, 2] = -np.abs(G[:, :, 2])
    G = bf16_round(G.astype(np.float32))
    if signed:      # bf16 rounding moved s G by 2^-8 relative at most: the denominator stays above 1
        assert np.all(np.where(G > 0, 2 + s[:, None, :] * G, 2) >= 1)
    return A.astype(np.float32), G


def synth_clstm(B, T, hid, plane, steps, seed, signed):
    """The same in the ConvLSTM layout: feat, grad [B, T, hid, plane]; the statistics are those of the selected steps,
    the other steps hold values the reduction must not read into its sums."""
    n = len(steps)
    A, G = synth(B, n * plane, hid, seed, signed)
    rng = np.random.default_rng(seed + 7919)
    feat = bf16_round(rng.normal(0, 3, (B, T, hid, plane)).astype(np.float32))
    grad = bf16_round(rng.normal(0, 3, (B, T, hid, plane)).astype(np.float32))
    feat[:, list(steps)] = A.reshape(B, n, plane, hid).transpose(0, 1, 3, 2)
    grad[:, list(steps)] = G.reshape(B, n, plane, hid).transpose(0, 1, 3, 2)
    return feat, grad


# the shapes of the direct kernel test (tests/test_gpu_cam.py) that the host tests check the gate and the mutants on
HOST_CASES = [(1, 1, 1), (3, 2040, 64), (2, 540, 480), (1, 65, 6), (2, 257, 68), (2, 8, 1024)]


def preconditions(A, G, kinds=KINDS):
    """What a case must satisfy for its test to mean something: dict(clamped={kind: fraction of the positions with a
    non-zero sum that the final ReLU clamps}, pp_den_min=min |2 + s G| over G > 0, s_ratio_min=min over s_k != 0 of |s_k| / sum|A|)."""
    A = np.asarray(A, np.float64)
    G = np.asarray(G, np.float64)
    f = family(A, G, kinds)
    s, sa = A.sum(axis=0), np.abs(A).sum(axis=0)
    d = np.abs(2 + s[None] * G)[G > 0]
    nz = s != 0
    def clamped(pre):          # of the positions whose sum is not exactly 0 (no gradient there, or a dead window)
        nz = pre != 0
        return float(np.mean(pre[nz] < 0)) if nz.any() else 0.0
    return dict(clamped={k: clamped(f[k]["pre"]) for k in kinds},
                pp_den_min=float(d.min()) if d.size else np.inf,
                s_ratio_min=float((np.abs(s[nz]) / sa[nz]).min()) if nz.any() else np.inf,
                sg=(s[None] * G))


def finish_maps(cam, clip_size, width, height, per_frame):
    """Raw maps [T', h, w] -> the final [T, H, W] float32 maps, by the arithmetic of the reference's GradCamVideo
    (grad_cam_videos.py:113-138) as oracle.gradcam_ref.cam_from_activations restates it: bilinear resize per slice,
    repeat T // T' frames, min/max normalisation per slice block or per clip (0/0 -> NaN)."""
    from oracle.gradcam_ref import resize_bilinear
    cam = np.asarray(cam, np.float32)
    step = clip_size // cam.shape[0]
    vid = np.array([np.repeat(resize_bilinear(c, width, height)[None], step, axis=0) for c in cam])
    with np.errstate(invalid='ignore', divide='ignore'):
        if per_frame:
            for i in range(vid.shape[0]):
                vid[i] = vid[i] - np.min(vid[i])
                vid[i] = vid[i] / np.max(vid[i])
        else:
            vid = vid - np.min(vid)
            vid = vid / np.max(vid)
    return vid.reshape((-1,) + vid.shape[2:]).astype(np.float32)
