"""References and derived bounds for the exhaustive one-box search (maskType 'stcombi', csrc/stmask_ops.hip):
test_gpu_box.py on the GPU, test_box_refs_host.py on the CPU.  Nothing here needs a GPU.

Candidates.  (a, L, i0, bh, j0, bw): frames [a, a+L), grid rows [i0, i0+bh), grid columns [j0, j0+bw).  The three axes
are one-blob tables in the order of ivf_blob_count (length ascending, then start); k = (kt n_h + kh) n_w + kw.

Staging.  The contract is equality with ivf_stmask_expand_fwd + ivf_stfreeze_fwd on the explicit binary S, so the GPU
test needs no bound.  `stage32` restates the direct evaluation (box sums only) and `stage32_via_S` the two kernels' own
sums (every term, zeros included) in sequential IEEE float32 on the host; the host test proves the two equal, which is
the argument that the zero terms of the expand drop out exactly, and holds both to the fp64 reference within
stmask_refs' bounds.

Objective.  J = t1 + t2 + t3 + s with t_i = (lam_i n_i) / cells, n_i a small integer (exact in fp32) and lam_i the
float the C interface carries: each t_i is rounded twice (product, quotient) and then passes through at most three
additions, s through one to three:
    b_J = gamma(5) (t1 + t2 + t3 + |s|)                               (`objective_bound`).

Drop map.  drop = (sum over covering candidates of (orig - s_k)) / count in fp32, k ascending: the bound the issue sets,
    b_drop = gamma(count) sum |orig - s_k| / count                    (`drop_ref`).
"""
import numpy as np
import torch

import stmask_refs as SR
from mask_refs import gamma


def blob_table(size, max_len):
    return [(a, ln) for ln in range(1, max_len + 1) for a in range(size - ln + 1)]


def blob_count(size, max_len):
    return max_len * (size + 1) - max_len * (max_len + 1) // 2


def box_count(T, max_len, gh, gw, mh, mw):
    return blob_count(T, max_len) * blob_count(gh, mh) * blob_count(gw, mw)


def box_table(T, grid, max_len, max_box):
    """int64 [n,6], row k = (kt n_h + kh) n_w + kw"""
    gh, gw = grid
    rows = [t + h + w for t in blob_table(T, max_len) for h in blob_table(gh, max_box[0]) for w in blob_table(gw, max_box[1])]
    return np.asarray(rows, dtype=np.int64).reshape(-1, 6)


def box_index(c, T, grid, max_box):
    """tuple -> k (the inverse of box_table's order)"""
    gh, gw = grid
    a, L, i0, bh, j0, bw = (int(v) for v in c)

    def ax(size, lo, ln):
        return (ln - 1) * (size + 1) - (ln - 1) * ln // 2 + lo
    return (ax(T, a, L) * blob_count(gh, max_box[0]) + ax(gh, i0, bh)) * blob_count(gw, max_box[1]) + ax(gw, j0, bw)


def box_S(c, T, grid, drop_last_row=False):
    """explicit binary S [T,gh,gw] float32; drop_last_row: the mutant"""
    gh, gw = grid
    a, L, i0, bh, j0, bw = (int(v) for v in c)
    S = torch.zeros(T, gh, gw)
    S[a:a + L, i0:i0 + bh - (1 if drop_last_row else 0), j0:j0 + bw] = 1.0
    return S


# ------------------------------------------------------------------------------------------------ staging
def _freeze32(x, M):
    """stfreeze_fwd's expression in sequential float32: x [C,T,H,W], M [T,H,W] -> P [C,T,H,W]"""
    T = x.shape[1]
    frames = [x[:, 0]]
    one = torch.tensor(1.0)
    for u in range(1, T):
        m = M[u][None]
        frames.append((one - m) * x[:, u] + m * frames[-1])
    return torch.stack(frames, dim=1)


def stage32(x, c, AH, AW, swap=False, all_frames=False):
    """the staged clip of candidate c as the kernel evaluates it: box sums only, float32, ascending.  x [C,T,H,W].
    Mutants: swap (rows and columns of the box exchanged), all_frames (the recurrence with the blob's M on every frame)."""
    C, T, H, W = x.shape
    a, L, i0, bh, j0, bw = (int(v) for v in c)
    if swap:
        i0, bh, j0, bw = j0, bw, i0, bh
    rw = torch.zeros(W)
    for j in range(j0, j0 + bw):
        rw = rw + AW[:, j]
    m = torch.zeros(H, W)
    for i in range(i0, i0 + bh):
        m = m + AH[:, i][:, None] * rw[None, :]
    M = torch.zeros(T, H, W)
    if all_frames:
        M[:] = m
    else:
        M[a:a + L] = m
    return _freeze32(x, M)


def expand32(S, AH, AW):
    """stmask_expand_fwd_kernel's sums, every term, in sequential float32: S [T,gh,gw] -> M [T,H,W]"""
    T, gh, gw = S.shape
    tmp = torch.zeros(T, gh, AW.shape[0])
    for j in range(gw):
        tmp = tmp + S[:, :, j][:, :, None] * AW[:, j][None, None, :]
    M = torch.zeros(T, AH.shape[0], AW.shape[0])
    for i in range(gh):
        M = M + AH[:, i][None, :, None] * tmp[:, i][:, None, :]
    return M


def stage32_via_S(x, S, AH, AW):
    return _freeze32(x, expand32(S, AH, AW))


def stage64(x, S, AH, AW):
    """fp64: stmask_refs' expand and per-pixel freeze on the explicit S; x [C,T,H,W] -> [C,T,H,W]"""
    C, T, H, W = x.shape
    M = SR.expand64(S[None], AH, AW).reshape(1, T, H * W)
    return SR.stfreeze_fwd64(x.reshape(1, C, T, H * W), M).reshape(C, T, H, W)


def stage_inputs(b, C, T, H, W, key='box'):
    """clips in 0..255 whose frames, channels, rows and columns all differ (a value read from the wrong place moves the
    result), with noise"""
    g = SR._gen('boxstage', key, b, C, T, H, W)
    t = torch.arange(T, dtype=torch.float32).view(1, 1, T, 1, 1)
    c = torch.arange(C, dtype=torch.float32).view(1, C, 1, 1, 1)
    y = torch.arange(H, dtype=torch.float32).view(1, 1, 1, H, 1)
    xx = torch.arange(W, dtype=torch.float32).view(1, 1, 1, 1, W)
    base = 20.0 + 150.0 * t / max(T - 1, 1) + 17.0 * c + 2.0 * y + 1.0 * xx
    return (base + torch.rand(b, C, T, H, W, generator=g) * 30.0).float().contiguous()


# ------------------------------------------------------------------------------------------------ objective, selection
def box_reg(tab, T, grid):
    """(volume, TVt, TVs) int64 [n] of ivf_stmask_reg on the binary S of each row, in closed form"""
    gh, gw = grid
    a, L, i0, bh, j0, bw = (tab[:, q] for q in range(6))
    w = SR.tv_pairs(T).numpy().astype(np.int64) if T >= 2 else np.zeros(0, np.int64)      # pair (k, k+1) -> weight
    wt = np.zeros(len(tab), np.int64)
    lo, hi = a >= 1, a + L < T
    wt[lo] += w[a[lo] - 1]
    wt[hi] += w[(a + L - 1)[hi]]
    tvt = bh * bw * wt
    tvs = L * (bw * ((i0 >= 1).astype(np.int64) + (i0 + bh < gh)) + bh * ((j0 >= 1).astype(np.int64) + (j0 + bw < gw)))
    return L * bh * bw, tvt, tvs


def objective64(tab, scores, T, grid, lams):
    """J [b,n] float64 (lams as the floats the interface carries) and its fp32 gate"""
    cells = grid[0] * grid[1]
    l1, l2, l3 = (float(np.float32(v)) for v in lams)
    vol, tvt, tvs = box_reg(tab, T, grid)
    t = (l1 * vol + l2 * tvt + l3 * tvs) / cells
    tabs = (abs(l1) * vol + abs(l2) * tvt + abs(l3) * tvs) / cells
    s = np.asarray(scores, dtype=np.float64)
    return t[None] + s, gamma(5) * (tabs[None] + np.abs(s))


def objective32(tab, scores, T, grid, lams):
    """the device's own expression in IEEE float32 (numpy): bit-comparable"""
    f = np.float32
    cells = f(grid[0] * grid[1])
    vol, tvt, tvs = (v.astype(f) for v in box_reg(tab, T, grid))
    t1, t2, t3 = (f(lams[0]) * vol) / cells, (f(lams[1]) * tvt) / cells, (f(lams[2]) * tvs) / cells
    return ((t1 + t2)[None] + t3[None]) + np.asarray(scores, dtype=f)


def select_rule(J, scores, orig, full, tab, threshold):
    """best k [b] (argmin J, NaN skipped, smaller k on a tie, -1 if none) and minimal k [b] (smallest volume with some
    r >= threshold, largest r within it, then smaller k, -1 if none); r in IEEE float32 as the device computes it"""
    f = np.float32
    b, n = J.shape
    vol = tab[:, 1] * tab[:, 3] * tab[:, 5]
    best, minimal = np.full(b, -1, np.int64), np.full(b, -1, np.int64)
    for r_ in range(b):
        ok = ~np.isnan(J[r_])
        if ok.any():
            best[r_] = int(np.flatnonzero(ok)[np.argmin(J[r_][ok], )])        # argmin returns the first minimum
        with np.errstate(invalid='ignore', divide='ignore'):
            r = (f(orig[r_]) - np.asarray(scores[r_], f)) / (f(orig[r_]) - f(full[r_]))
        q = np.flatnonzero(r >= f(threshold))
        if q.size:
            q = q[vol[q] == vol[q].min()]
            q = q[r[q] == r[q].max()]
            minimal[r_] = int(q[0])
    return best, minimal


# ------------------------------------------------------------------------------------------------ drop map
def drop_brute(scores, orig, tab, T, grid):
    """(sum64, count, sum|.|) [b,T,gh,gw] by a loop over ALL candidates and all cells"""
    gh, gw = grid
    b = scores.shape[0]
    sm, cnt, sab = (np.zeros((b, T, gh, gw)) for _ in range(3))
    for k, (a, L, i0, bh, j0, bw) in enumerate(tab):
        for t in range(T):
            for i in range(gh):
                for j in range(gw):
                    if a <= t < a + L and i0 <= i < i0 + bh and j0 <= j < j0 + bw:
                        for r in range(b):
                            s = float(scores[r, k])
                            if s == s:
                                sm[r, t, i, j] += float(orig[r]) - s
                                sab[r, t, i, j] += abs(float(orig[r]) - s)
                                cnt[r, t, i, j] += 1
    return sm, cnt, sab


def drop_ref(scores, orig, tab, T, grid):
    """fp64 drop map [b,T,gh,gw], its gate and the counts, by box slices (the host test holds it to drop_brute)"""
    gh, gw = grid
    s = np.asarray(scores, np.float64)
    b = s.shape[0]
    d = np.asarray(orig, np.float64)[:, None] - s
    ok = ~np.isnan(d)
    d = np.where(ok, d, 0.0)
    sm, cnt, sab = (np.zeros((b, T, gh, gw)) for _ in range(3))
    for k, (a, L, i0, bh, j0, bw) in enumerate(tab):
        sl = (slice(None), slice(a, a + L), slice(i0, i0 + bh), slice(j0, j0 + bw))
        sm[sl] += d[:, k, None, None, None]
        sab[sl] += np.abs(d[:, k, None, None, None])
        cnt[sl] += ok[:, k, None, None, None]
    with np.errstate(invalid='ignore', divide='ignore'):
        return sm / cnt, gamma(np.maximum(cnt, 1)) * sab / np.maximum(cnt, 1), cnt
