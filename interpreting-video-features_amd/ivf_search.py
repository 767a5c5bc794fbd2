"""Batched per-clip mask search on top of a network engine (I3D or CLSTM_4).

One call runs, for b DIFFERENT clips with b DIFFERENT masks, what the reference
runs for one `batch_index` at a time (FindMasksComparison_I3D_smth.py:166-277):
baseline scores -> init_mask('central') -> N Adam iterations -> reverse score ->
Grad-CAM.  In eval mode the rows of a batch are independent, so
per clip the numbers are the ones the reference computes.

Everything that computes is a libivf_hip call; this file only sequences them
and makes the handful of host decisions the reference makes on the host
(which central mask to keep, mask.py:134-147).
"""
import numpy as np
import torch

import ivf_lib as L


def central_masks(T, device):
    """mask.py:135-137 for i = 1 .. T//2-1: ones with i zeros at each end."""
    rows = []
    for i in range(1, T // 2):
        m = torch.ones(T)
        m[:i] = 0
        m[T - i:] = 0
        rows.append(m)
    return torch.stack(rows).to(device)


def init_masks_central(engine, x, target, orig_score, threshold=0.9, mask_type="freeze"):
    """mask.init_mask(mode='central'), mask.py:121-154, for b clips at once.
    Returns (raw masks [b,T] in {-5,+5}, info dict).  The reference stops at the
    first i whose score ratio drops below `threshold`; here all T//2-1 candidates are
    scored (<= 6 extra forwards per clip) and the same i is selected afterwards, so
    the loop needs one host sync instead of one per candidate."""
    b, _, T = x.shape[0], x.shape[1], x.shape[2]
    dev = x.device
    idx = torch.arange(b, device=dev)
    tl = target.long()
    # the fully perturbed clip is ALWAYS the fully frozen one (mask.py:123-128), whatever mask_type
    full = engine.perturbed_forward(x, torch.ones(b, T, device=dev), "freeze")[idx, tl]
    cands = central_masks(T, dev)
    cen = torch.stack([engine.perturbed_forward(x, cands[i][None].expand(b, T).contiguous(), mask_type)[idx, tl]
                       for i in range(cands.shape[0])], dim=1)                                # :139-141
    n = cands.shape[0]
    orig = L.f32c(orig_score)
    full, cen = L.f32c(full), L.f32c(cen)
    raw = torch.empty(b, T, device=dev)
    first = torch.empty(b, dtype=torch.int32, device=dev)
    ratio = torch.empty(b, n, device=dev)
    with torch.cuda.device(dev):                                                               # :142-154
        L.check(L.lib().ivf_init_central_select(L.ptr(orig), L.ptr(full), L.ptr(cen), b, n, T, float(threshold),
                                                L.ptr(raw), L.ptr(first), L.ptr(ratio), L.stream()))
    return raw, dict(full=full, central=cen, ratio=ratio, chosen_i=first.long())


def find_submasks_host(mask_row, thresh=0.1):
    """Host view of the integer output of ivf_submask_pairs for one mask."""
    T = mask_row.numel()
    m = L.f32c(mask_row.detach().reshape(-1))
    L.require_gpu(m)
    run = torch.empty(T, dtype=torch.int32, device=m.device)
    partner = torch.empty(T, dtype=torch.int32, device=m.device)
    weight = torch.empty(T, device=m.device)
    with torch.cuda.device(m.device):
        L.check(L.lib().ivf_submask_pairs(L.ptr(m), T, float(thresh), L.ptr(run), L.ptr(partner), L.ptr(weight),
                                          L.stream()))
    runs = {}
    for t, r in enumerate(run.cpu().tolist()):
        if r >= 0:
            runs.setdefault(r, []).append(t)
    return [runs[r] for r in sorted(runs)]


def frame_ranking(mask):
    """Integer frame-importance ranking: stable argsort of -mask (ivf_rank_frames)."""
    m = L.f32c(mask.detach())
    L.require_gpu(m)
    T = m.shape[-1]
    order = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    with torch.cuda.device(m.device):
        L.check(L.lib().ivf_rank_frames(L.ptr(m), m.numel() // T, T, L.ptr(order), L.stream()))
    return order.long()


def blob_candidates(T, max_len=None):
    """The one-blob candidates of maskType 'combi' (smth:137-141) as a host int64 table [n, 2] of (a, L): every
    binary mask that is 1 on [a, a+L), 1 <= L <= max_len (default T), in canonical order (L, then a)."""
    ml = T if max_len is None else int(max_len)
    n = L.lib().ivf_blob_count(int(T), ml)
    if n < 0:
        raise L.IvfError(L.lib().ivf_last_error().decode())
    rows = [(a, ln) for ln in range(1, ml + 1) for a in range(T - ln + 1)]
    return torch.tensor(rows, dtype=torch.int64).reshape(n, 2)


def blob_select(scores, orig, full, T, max_len=None, lam1=0.01, lam2=0.02, threshold=0.9, want_obj=False):
    """ivf_blob_select on a score grid [b, n]: dict of device tensors best [b,2] (a, L of argmin J), objective [b]
    (its J), minimal [b,2] (smallest sufficient blob, (-1,-1) if none) and, with want_obj, obj [b,n]."""
    s = L.f32c(scores)
    L.require_gpu(s)
    b = s.shape[0]
    ml = T if max_len is None else int(max_len)
    orig, full = L.f32c(orig.reshape(b)), L.f32c(full.reshape(b))
    best = torch.empty(b, 2, dtype=torch.int32, device=s.device)
    minimal = torch.empty(b, 2, dtype=torch.int32, device=s.device)
    bobj = torch.empty(b, device=s.device)
    obj = torch.empty_like(s) if want_obj else None
    with torch.cuda.device(s.device):
        L.check(L.lib().ivf_blob_select(L.ptr(s), L.ptr(orig), L.ptr(full), b, int(T), ml, float(lam1), float(lam2),
                                        float(threshold), L.ptr(best), L.ptr(bobj), L.ptr(obj), L.ptr(minimal),
                                        L.stream()))
    out = dict(best=best.long(), objective=bobj, minimal=minimal.long())
    if want_obj:
        out["obj"] = obj
    return out


def blob_index(blob, T):
    """Grid column k(a, L) = sum_{l<L} (T-l+1) + a of (a, L) rows [b,2]; -1 where L < 1."""
    a, ln = blob[:, 0], blob[:, 1]
    k = (ln - 1) * (T + 1) - (ln - 1) * ln // 2 + a
    return torch.where(ln >= 1, k, torch.full_like(k, -1))


def blob_masks(best, T):
    """Binary float masks [b, T] of (a, L) rows [b, 2]: 1 on [a, a+L) (all zero for L < 1)."""
    u = torch.arange(T, device=best.device)[None]
    a, ln = best[:, :1], best[:, 1:]
    return ((u >= a) & (u < a + ln)).float()


def _box_limits(T, grid, max_len, max_box):
    gh, gw = (int(v) for v in grid)
    ml = int(T) if max_len is None else int(max_len)
    mh, mw = (gh, gw) if max_box is None else (int(v) for v in max_box)
    n = L.lib().ivf_box_count(int(T), ml, gh, gw, mh, mw)
    if n < 0:
        raise L.IvfError(L.lib().ivf_last_error().decode())
    return gh, gw, ml, mh, mw, n


def box_candidates(T, grid, max_len=None, max_box=None):
    """The one-box candidates of maskType 'stcombi' as a host int64 table [n, 6] of (a, L, i0, bh, j0, bw): frames
    [a, a+L), grid rows [i0, i0+bh), grid columns [j0, j0+bw), L <= max_len (default T), (bh, bw) <= max_box (default
    the grid).  Row k = (kt * n_h + kh) * n_w + kw, each axis in the order of blob_candidates."""
    gh, gw, ml, mh, mw, n = _box_limits(T, grid, max_len, max_box)
    t, h, w = blob_candidates(T, ml), blob_candidates(gh, mh), blob_candidates(gw, mw)
    nt, nh, nw = t.shape[0], h.shape[0], w.shape[0]
    out = torch.cat([t[:, None, None, :].expand(nt, nh, nw, 2), h[None, :, None, :].expand(nt, nh, nw, 2),
                     w[None, None, :, :].expand(nt, nh, nw, 2)], dim=3)
    return out.reshape(n, 6).contiguous()


def box_select(scores, orig, full, T, grid, max_len=None, max_box=None, lam1=0.01, lam2=0.02, lam3=None, threshold=0.9,
               want_obj=False):
    """ivf_box_select on a score grid [b, n]: dict of device tensors best [b,6] (a, L, i0, bh, j0, bw of argmin J),
    objective [b] (its J), minimal [b,6] (smallest sufficient box, all -1 if none), index [b] (k of best, -1 if none)
    and, with want_obj, obj [b,n].  lam3 defaults to lam2."""
    gh, gw, ml, mh, mw, n = _box_limits(T, grid, max_len, max_box)
    s = L.f32c(scores)
    L.require_gpu(s)
    b = s.shape[0]
    if tuple(s.shape) != (b, n):
        raise L.IvfError(f"scores must be [b,{n}], got {tuple(s.shape)}")
    orig, full = L.f32c(orig.reshape(b)), L.f32c(full.reshape(b))
    best = torch.empty(b, 6, dtype=torch.int32, device=s.device)
    minimal = torch.empty(b, 6, dtype=torch.int32, device=s.device)
    bobj = torch.empty(b, device=s.device)
    obj = torch.empty_like(s) if want_obj else None
    with torch.cuda.device(s.device):
        L.check(L.lib().ivf_box_select(L.ptr(s), L.ptr(orig), L.ptr(full), b, int(T), gh, gw, ml, mh, mw, float(lam1),
                                       float(lam2), float(lam2 if lam3 is None else lam3), float(threshold), L.ptr(best),
                                       L.ptr(bobj), L.ptr(obj), L.ptr(minimal), L.stream()))
    best = best.long()
    nh, nw = L.lib().ivf_blob_count(gh, mh), L.lib().ivf_blob_count(gw, mw)
    k = (blob_index(best[:, 0:2], int(T)) * nh + blob_index(best[:, 2:4], gh)) * nw + blob_index(best[:, 4:6], gw)
    out = dict(best=best, objective=bobj, minimal=minimal.long(), index=torch.where(best[:, 1] >= 1, k, torch.full_like(k, -1)))
    if want_obj:
        out["obj"] = obj
    return out


def box_drop(scores, orig, T, grid, max_len=None, max_box=None):
    """ivf_box_drop: the occlusion map [b,T,gh,gw] of a score grid [b,n] -- per cell the mean of orig - score over the
    candidates whose box covers it."""
    gh, gw, ml, mh, mw, n = _box_limits(T, grid, max_len, max_box)
    s = L.f32c(scores)
    L.require_gpu(s)
    b = s.shape[0]
    if tuple(s.shape) != (b, n):
        raise L.IvfError(f"scores must be [b,{n}], got {tuple(s.shape)}")
    orig = L.f32c(orig.reshape(b))
    drop = torch.empty(b, int(T), gh, gw, device=s.device)
    with torch.cuda.device(s.device):
        L.check(L.lib().ivf_box_drop(L.ptr(s), L.ptr(orig), b, int(T), gh, gw, ml, mh, mw, L.ptr(drop), L.stream()))
    return drop


def box_masks(best, T, grid):
    """Binary float S [b,T,gh,gw] of (a, L, i0, bh, j0, bw) rows [b,6] (all zero for L < 1)."""
    gh, gw = (int(v) for v in grid)
    dev = best.device

    def axis(n, lo, ln):
        u = torch.arange(n, device=dev)[None]
        return ((u >= lo[:, None]) & (u < (lo + ln)[:, None])).float()
    t, h, w = axis(int(T), best[:, 0], best[:, 1]), axis(gh, best[:, 2], best[:, 3]), axis(gw, best[:, 4], best[:, 5])
    return (t[:, :, None, None] * h[:, None, :, None] * w[:, None, None, :]).contiguous()


def frame_means(S):
    """Spatial mean per frame [b,T] of S [b,T,gh,gw]: ivf_stmask_expand_fwd onto a single pixel (H = W = 1) with the
    uniform rows 1/gh, 1/gw as its two matrices -- the same fixed-order sums as everywhere else, no new kernel (see
    ivf_hip.h)."""
    b, T, gh, gw = S.shape
    dev = S.device
    mean = torch.empty(b, T, device=dev)
    ah, aw = torch.full((1, gh), 1.0 / gh, device=dev), torch.full((1, gw), 1.0 / gw, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().ivf_stmask_expand_fwd(L.ptr(S), L.ptr(ah), L.ptr(aw), L.ptr(mean), b, T, gh, gw, 1, 1, L.stream()))
    return mean


def score_at(scores, k):
    """scores[i, k[i]] of a score grid [b,n]; NaN where k[i] < 0 (no candidate picked)."""
    b = scores.shape[0]
    idx = torch.arange(b, device=scores.device)
    return torch.where(k >= 0, scores[idx, k.clamp(min=0)], torch.full((b,), float("nan"), device=scores.device))


def time_mask_outputs(eng, x, target, mask, out):
    """From a time_mask [b,T]: the score of the reversed clip (smth:234-235), the frame ranking and the snapped mask
    (mask.py:5-10)."""
    idx = torch.arange(x.shape[0], device=x.device)
    out["reverse_score"] = eng.perturbed_forward(x, mask, "reverse")[idx, target.long()]
    out["ranking"] = frame_ranking(mask)
    out["snapped"] = mask > 0.5


class MaskSearch:
    def __init__(self, engine, lam1=0.01, lam2=0.02, n_iter=300, mask_type="freeze", threshold=0.9,
                 lr=0.2, grad_cam_type="guessed", do_gradcam=True, run_temp_mask=True,
                 normalize_per_frame=True, gradcam_size=None, mask_mode="central", max_mask_length=None,
                 mask_grid=None, mask_sigma=None, lam3=None, max_box=None, do_intgrad=False, ig_steps=32,
                 ig_baseline="frozen", do_rise=False, rise_masks=1024, rise_p=0.5, rise_grid=None, rise_sigma=None,
                 rise_seed=0, do_smoothgrad=False, sg_samples=32, sg_level=0.15, sg_seed=0, do_shapley=False,
                 shap_perms=64, shap_grid=None, shap_sigma=None, shap_seed=0, do_curves=False, curve_grid=None,
                 curve_sigma=None, curve_step=1, cam_kinds=(), cam_target=None, do_scorecam=False, scorecam_target=None,
                 scorecam_weights="increase", scorecam_perturb="freeze", scorecam_sigma=None, scorecam_channels=None,
                 do_kernelshap=False, kshap_samples=256, kshap_grid=None, kshap_sigma=None, kshap_seed=0, do_lime=False,
                 lime_samples=1024, lime_p=0.5, lime_grid=None, lime_sigma=None, lime_seed=0, lime_width=0.25,
                 lime_ridge=1.0):
        """do_kernelshap, do_lime (extensions without a counterpart in the reference): also fit a linear
        surrogate of the target's score drop in the frozen cells of kshap_grid / lime_grid (gt, gh, gw) (default
        (T, 1, 1): the frames), blurred by kshap_sigma / lime_sigma input pixels, forward passes only, the fit in fp64 on
        the device.  KernelSHAP: kshap_samples paired coalitions with Shapley-kernel sizes drawn from kshap_seed, the
        efficiency constraint solved exactly; run() then also returns kshap_map [b,T,H,W], kshap_cells [b,gt,gh,gw],
        kshap_frames [b,T], kshap_total, kshap_ok and kshap_r2 [b].  LIME: lime_samples Bernoulli(lime_p) rows drawn
        from lime_seed, weighted by an exponential kernel of width lime_width, ridge lime_ridge, a free intercept; run()
        then also returns lime_map, lime_cells, lime_frames, lime_intercept, lime_ok and lime_r2.  do_curves ranks the
        maps under 'kshap' and 'lime'.  The perturbation is the per-pixel freeze only.
        do_scorecam (an extension without a counterpart in the reference): also run Score-CAM of the
        target's score on scorecam_target (an endpoint name, or the ConvLSTM engine's layer; default: the Grad-CAM
        target) -- every channel (or the window scorecam_channels = (first, count)) normalised, expanded to the clip
        (blurred by scorecam_sigma input pixels) and applied as scorecam_perturb ('freeze' or 'blank'), weighted as
        scorecam_weights ('increase' or 'softmax'), forward passes only; run() then also returns scorecam_map
        [b,frames,H,W] (resized and normalised as the Grad-CAM map), scorecam_cam, scorecam_weights, scorecam_valid and
        scorecam_score_base [b], and do_curves ranks the map under 'scorecam'.
        cam_kinds (an extension without a counterpart in the reference; with do_gradcam): further members
        of the activation-map family -- 'gradcam++', 'xgradcam', 'hirescam', 'layercam' -- on cam_target (an endpoint
        name, or the ConvLSTM engine's layer; default: the Grad-CAM target, and then Grad-CAM and the extra kinds come
        from ONE forward and ONE backward); run() then also returns cam_<kind> [b,T,H,W], and do_curves ranks them under
        the kind's name.
        do_curves (an extension without a counterpart in the reference): also run the deletion and
        insertion curves (Petsiuk et al. 2018) of every attribution this call produced, on the cells of curve_grid
        (gt, gh, gw) (default (T, 1, 1): the frames), blurred by curve_sigma input pixels, curve_step cells per forward.
        With a frame grid (gh = gw = 1) the attributions are the frame profiles -- time_mask (named 'st_mask' where it
        is the frame means of st_mask), the per-frame mean of the Grad-CAM map, ig_frames, rise_frames, sg_frames,
        shap_frames; with a spatial grid they are the [T,H,W] maps (the expanded st_mask, gradcam, ig_map, rise_map,
        sg_map, shap_map) and a method without one is left out.  'random' (the expected curves of a random order, at
        step 1) is added when Shapley ran on the same grid and sigma.  run() then also returns, per method m,
        curves_<m>_ranks [b,P] (not for 'random'), curves_<m>_deletion, curves_<m>_insertion [b,J+1],
        curves_<m>_del_auc, _ins_auc, _del_auc_norm, _ins_auc_norm [b].  The perturbation is the per-pixel freeze only.
        do_shapley (an extension without a counterpart in the reference): also run Shapley value sampling
        of the target's score -- shap_perms permutations (every odd one the reverse of the one before) of the cells of
        shap_grid (gt, gh, gw) (default (T, 1, 1): the frames), blurred by shap_sigma input pixels, drawn from
        shap_seed, forward passes only; run() then also returns shap_map [b,T,H,W], shap_cells, shap_stderr, shap_count
        [b,gt,gh,gw], shap_frames [b,T] and shap_total [b].  The perturbation is the per-pixel freeze only.
        do_smoothgrad (an extension without a counterpart in the reference): also run SmoothGrad,
        SmoothGrad^2 and VarGrad of the target's score -- sg_samples noisy copies of each clip, noise of standard
        deviation sg_level * (max(clip) - min(clip)) drawn from sg_seed, one forward and backward each; run() then also
        returns sg_map, sg_sq_map, sg_var_map [b,T,H,W], sg_frames [b,T] and sg_sigma [b].
        do_rise (an extension without a counterpart in the reference): also run RISE random-mask saliency
        of the target's score -- rise_masks random masks on rise_grid (gt, gh, gw) (default (min(T, 8),) + the spatial
        grid of 'spacetime'), each cell frozen with probability rise_p, blurred by rise_sigma input pixels, drawn from
        rise_seed; run() then also returns rise_map [b,T,H,W], rise_cells, rise_count [b,gt,gh,gw], rise_frames [b,T]
        and rise_mean_drop [b].  The perturbation is the per-pixel freeze only.
        do_intgrad (an extension without a counterpart in the reference): also run Integrated Gradients
        of the target's score with ig_steps midpoint nodes from the ig_baseline ('frozen': every frame = frame 0, the
        fully frozen clip of mask.py:123-128; 'constant': black); run() then also returns ig_map [b,T,H,W], ig_frames
        [b,T], ig_abs_frames, ig_total, ig_gap and ig_score_base [b].
        mask_mode 'central': init_mask('central') + n_iter Adam steps (smth:188-214); 'combi': the exhaustive
        one-blob search (smth:137-141) over masks of length <= max_mask_length (default T), no gradient descent;
        'spacetime' (an extension without a counterpart in the reference): the gradient search on a mask per
        frame and grid cell -- mask_grid (gh, gw) (default one cell per 32 input pixels: 7x7 at 224^2, 4x5 at
        120x160), mask_sigma the blur in input pixels (default 0.5 H / gh), lam3 the spatial TV weight (default lam2);
        the perturbation is the per-pixel freeze.  'stcombi'  is to 'spacetime' what 'combi' is to 'central':
        every box of one temporal blob (length <= max_mask_length) times one rectangle of grid cells (at most max_box =
        (mh, mw), default the whole grid) is scored by a forward pass and the minimiser of the spacetime loss picked on
        the device; mask_grid, mask_sigma and lam3 as for 'spacetime', n_iter unused."""
        if mask_mode not in ("central", "combi", "spacetime", "stcombi"):
            raise L.IvfError(f"mask_mode must be 'central', 'combi', 'spacetime' or 'stcombi', got {mask_mode!r}")
        if mask_mode in ("spacetime", "stcombi") and mask_type != "freeze":
            raise L.IvfError(f"mask_mode {mask_mode!r} perturbs by freezing only")
        self.mask_mode, self.max_mask_length, self.max_box = mask_mode, max_mask_length, max_box
        self.mask_grid, self.mask_sigma, self.lam3 = mask_grid, mask_sigma, lam3
        self.engine = engine
        self.lam1, self.lam2, self.n_iter = float(lam1), float(lam2), int(n_iter)
        self.mask_type, self.threshold, self.lr = mask_type, threshold, lr
        self.grad_cam_type = grad_cam_type
        self.do_gradcam, self.run_temp_mask = do_gradcam, run_temp_mask
        self.cam_kinds, self.cam_target = L.cam_kind_ids(cam_kinds)[0], cam_target
        if "gradcam" in self.cam_kinds:
            raise L.IvfError("cam_kinds lists the kinds beside 'gradcam', which do_gradcam computes")
        self.normalize_per_frame = normalize_per_frame
        self.gradcam_size = gradcam_size
        self.do_intgrad, self.ig_steps, self.ig_baseline = bool(do_intgrad), ig_steps, ig_baseline   # read only when on
        if self.do_intgrad and ig_baseline not in ("frozen", "constant"):
            raise L.IvfError(f"ig_baseline must be 'frozen' or 'constant', got {ig_baseline!r}")
        self.do_rise = bool(do_rise)                                                                  # read only when on
        self.rise_masks, self.rise_p, self.rise_grid = rise_masks, rise_p, rise_grid
        self.rise_sigma, self.rise_seed = rise_sigma, rise_seed
        if self.do_rise and mask_type != "freeze":
            raise L.IvfError("RISE perturbs by freezing only")
        self.do_smoothgrad = bool(do_smoothgrad)                                                      # read only when on
        self.sg_samples, self.sg_level, self.sg_seed = sg_samples, sg_level, sg_seed
        self.do_shapley = bool(do_shapley)                                                            # read only when on
        self.shap_perms, self.shap_grid, self.shap_sigma, self.shap_seed = shap_perms, shap_grid, shap_sigma, shap_seed
        if self.do_shapley and mask_type != "freeze":
            raise L.IvfError("Shapley value sampling perturbs by freezing only")
        self.do_kernelshap, self.do_lime = bool(do_kernelshap), bool(do_lime)                         # read only when on
        self.kshap_samples, self.kshap_grid, self.kshap_sigma, self.kshap_seed = kshap_samples, kshap_grid, kshap_sigma, kshap_seed
        self.lime_samples, self.lime_p, self.lime_grid, self.lime_sigma = lime_samples, lime_p, lime_grid, lime_sigma
        self.lime_seed, self.lime_width, self.lime_ridge = lime_seed, lime_width, lime_ridge
        if self.do_kernelshap and mask_type != "freeze":
            raise L.IvfError("KernelSHAP perturbs by freezing only")
        if self.do_lime and mask_type != "freeze":
            raise L.IvfError("LIME perturbs by freezing only")
        self.do_curves = bool(do_curves)                                                              # read only when on
        self.curve_grid, self.curve_sigma, self.curve_step = curve_grid, curve_sigma, curve_step
        if self.do_curves and mask_type != "freeze":
            raise L.IvfError("deletion / insertion curves perturb by freezing only")
        self.do_scorecam = bool(do_scorecam)                                                          # read only when on
        self.scorecam_target, self.scorecam_weights, self.scorecam_perturb = scorecam_target, scorecam_weights, scorecam_perturb
        self.scorecam_sigma, self.scorecam_channels = scorecam_sigma, scorecam_channels
        if self.do_scorecam:
            engine._scorecam_kind(engine.SCORECAM_WEIGHTS, "weights", scorecam_weights)
            engine._scorecam_kind(engine.SCORECAM_PERTURB, "perturb", scorecam_perturb)

    def run(self, x, labels, want_traj=False):
        """x [b,C,T,H,W] float32 on the GPU, labels [b] ints.  Returns a dict of device
        tensors, one row per clip (nothing is copied to the host here)."""
        eng = self.engine
        b = x.shape[0]
        dev = x.device
        labels = torch.as_tensor(labels, device=dev).to(torch.int32).reshape(-1)
        out = {}
        probs = eng.forward(x)                                               # smth:176
        pred = eng.argmax(probs)                                             # smth:181 / :217
        target = pred if self.grad_cam_type == "guessed" else labels         # smth:179-184
        idx = torch.arange(b, device=dev)
        out["pred_class"] = pred
        out["target"] = target
        out["original_score_guess"] = probs[idx, pred.long()]
        out["original_score_true"] = probs[idx, labels.long()]
        if self.run_temp_mask and self.mask_mode == "combi":
            self._run_combi(x, target, probs, out)
        elif self.run_temp_mask and self.mask_mode == "spacetime":
            self._run_spacetime(x, target, probs, out, want_traj)
        elif self.run_temp_mask and self.mask_mode == "stcombi":
            self._run_stcombi(x, target, probs, out)
        elif self.run_temp_mask:
            raw, info = init_masks_central(eng, x, target, probs[idx, target.long()], self.threshold,
                                           self.mask_type)                   # smth:188-190
            out["init_mask"] = raw.clone()
            traj, _ = eng.search(x, target, raw, self.lam1, self.lam2, self.n_iter, lr=self.lr,
                                 want_traj=True, mode=self.mask_type)        # smth:191-214
            mask = torch.empty_like(raw)                                     # smth:216, with the sigmoid the loop itself uses
            with torch.cuda.device(dev):
                L.check(L.lib().ivf_sigmoid(L.ptr(raw), L.ptr(mask), raw.numel(), L.stream()))
            out["time_mask"] = mask
            out["freeze_score"] = traj[-1, :, 3] if self.n_iter > 0 else torch.full((b,), float("nan"), device=dev)
            time_mask_outputs(eng, x, target, mask, out)
            if want_traj:
                out["traj"] = traj
        if self.do_gradcam:
            gc_target = pred if self.grad_cam_type == "guessed" else target  # smth:253,266-267
            kw = dict(per_frame=self.normalize_per_frame, out_hw=self.gradcam_size)
            if self.cam_kinds and self.cam_target is None:                   # the family from Grad-CAM's own passes
                cams, _ = eng.cam(x, gc_target, kinds=["gradcam"] + self.cam_kinds, **kw)
                cam = cams["gradcam"]
            else:
                cam, _ = eng.gradcam(x, gc_target, **kw)
                if self.cam_kinds:
                    cams, _ = eng.cam(x, gc_target, kinds=self.cam_kinds, layer=self.cam_target, **kw)
            out["gradcam"] = cam                                             # smth:269
            for k in self.cam_kinds:
                out["cam_" + k] = cams[k]
        if self.do_intgrad:
            r = eng.ig(x, target, steps=self.ig_steps, baseline=self.ig_baseline)
            for k in ("ig_map", "ig_frames", "ig_abs_frames", "ig_total", "ig_gap"):
                out[k] = r[k]
            out["ig_score_base"] = r["score_base"]
        if self.do_scorecam:
            sc = eng.scorecam(x, target, layer=self.scorecam_target, weights=self.scorecam_weights,
                              perturb=self.scorecam_perturb, sigma=self.scorecam_sigma, channels=self.scorecam_channels,
                              per_frame=self.normalize_per_frame, out_hw=self.gradcam_size)
            for k in ("scorecam_map", "scorecam_cam", "scorecam_weights", "scorecam_valid"):
                out[k] = sc[k]
            out["scorecam_score_base"] = sc["score_base"]
        if self.do_rise:
            grid = self.rise_grid
            if grid is None:
                grid = (min(x.shape[2], 8),) + self.st_grid(x)
            r = eng.rise(x, target, n_masks=self.rise_masks, p=self.rise_p, grid=grid, sigma=self.rise_sigma,
                         seed=self.rise_seed)
            for k in ("rise_map", "rise_cells", "rise_count", "rise_frames", "rise_mean_drop"):
                out[k] = r[k]
        if self.do_smoothgrad:
            r = eng.smoothgrad(x, target, n_samples=self.sg_samples, level=self.sg_level, seed=self.sg_seed)
            out["sg_map"], out["sg_sq_map"], out["sg_var_map"] = r["sg_map"], r["sq_map"], r["var_map"]
            out["sg_frames"], out["sg_sigma"] = r["sg_frames"], r["sigma"]
        if self.do_shapley:
            r = eng.shapley(x, target, n_perms=self.shap_perms, grid=self.shap_grid, sigma=self.shap_sigma,
                            seed=self.shap_seed)
            for k in ("shap_map", "shap_cells", "shap_stderr", "shap_count", "shap_frames", "shap_total"):
                out[k] = r[k]
        if self.do_kernelshap:
            ks = eng.kernelshap(x, target, n_samples=self.kshap_samples, grid=self.kshap_grid, sigma=self.kshap_sigma,
                                seed=self.kshap_seed)
            for k in ("kshap_map", "kshap_cells", "kshap_frames", "kshap_total", "kshap_ok", "kshap_r2"):
                out[k] = ks[k]
        if self.do_lime:
            lm = eng.lime(x, target, n_samples=self.lime_samples, p=self.lime_p, grid=self.lime_grid, sigma=self.lime_sigma,
                          seed=self.lime_seed, width=self.lime_width, ridge=self.lime_ridge)
            for k in ("lime_map", "lime_cells", "lime_frames", "lime_intercept", "lime_ok", "lime_r2"):
                out[k] = lm[k]
        if self.do_curves:
            self._run_curves(x, target, out, r["shap_scores"] if self.do_shapley else None)
        return out

    def _curve_attributions(self, x, out, spatial):
        """{method: attribution} of what this call produced: frame profiles [b,T], or on a spatial grid [b,T,H,W] maps"""
        T, HW = x.shape[2], tuple(x.shape[3:])
        attrs = {}
        if spatial:
            if "st_mask" in out:
                attrs["st_mask"] = self.engine.st_expand(out["st_mask"], self.st_grid(x), self.mask_sigma)
            for name, key in [("gradcam", "gradcam"), ("ig", "ig_map"), ("rise", "rise_map"), ("sg", "sg_map"),
                              ("shap", "shap_map"), ("scorecam", "scorecam_map"), ("kshap", "kshap_map"),
                              ("lime", "lime_map")] + [(k, "cam_" + k) for k in self.cam_kinds]:
                if key in out and tuple(out[key].shape[1:]) == (T,) + HW:
                    attrs[name] = out[key]
            return attrs
        if "time_mask" in out:
            attrs["st_mask" if "st_mask" in out else "time_mask"] = out["time_mask"]
        if "gradcam" in out and out["gradcam"].shape[1] == T:
            attrs["gradcam"] = out["gradcam"].float().mean(dim=(2, 3))
        for k in self.cam_kinds:
            if out["cam_" + k].shape[1] == T:
                attrs[k] = out["cam_" + k].float().mean(dim=(2, 3))
        if "scorecam_map" in out and out["scorecam_map"].shape[1] == T:
            attrs["scorecam"] = out["scorecam_map"].float().mean(dim=(2, 3))
        for name, key in (("ig", "ig_frames"), ("rise", "rise_frames"), ("sg", "sg_frames"), ("shap", "shap_frames"),
                          ("kshap", "kshap_frames"), ("lime", "lime_frames")):
            if key in out:
                attrs[name] = out[key]
        return attrs

    def _run_curves(self, x, target, out, shap_scores):
        eng = self.engine
        T, H = x.shape[2], x.shape[3]
        grid = (T, 1, 1) if self.curve_grid is None else tuple(int(v) for v in self.curve_grid)
        if len(grid) != 3:
            raise L.IvfError(f"curve_grid must be (gt, gh, gw), got {self.curve_grid!r}")
        names = ("del_auc", "ins_auc", "del_auc_norm", "ins_auc_norm")
        for m, attr in self._curve_attributions(x, out, grid[1] > 1 or grid[2] > 1).items():
            r = eng.faithfulness(x, target, attr, grid=grid, sigma=self.curve_sigma, step=self.curve_step)
            out[f"curves_{m}_ranks"] = r["curve_ranks"]
            out[f"curves_{m}_deletion"], out[f"curves_{m}_insertion"] = r["del_scores"], r["ins_scores"]
            for k in names:
                out[f"curves_{m}_{k}"] = r[k]
        if shap_scores is not None:
            sgrid = (T, 1, 1) if self.shap_grid is None else tuple(int(v) for v in self.shap_grid)

            def blur(sigma, g):
                return 0.5 * H / g[1] if sigma is None else float(sigma)
            if sgrid == grid and blur(self.shap_sigma, sgrid) == blur(self.curve_sigma, grid):
                s = eng.curve_random_baseline(shap_scores)
                auc, norm = eng.curve_reduce(s, grid, 1, 3)
                out["curves_random_deletion"], out["curves_random_insertion"] = s[:, 0], s[:, 1]
                out["curves_random_del_auc"], out["curves_random_ins_auc"] = auc[:, 0], auc[:, 1]
                out["curves_random_del_auc_norm"], out["curves_random_ins_auc_norm"] = norm[:, 0], norm[:, 1]


    def _run_combi(self, x, target, probs, out):
        """maskType 'combi': score every one-blob mask, pick argmin of the search loss on the device."""
        eng = self.engine
        b, T = x.shape[0], x.shape[2]
        dev = x.device
        idx = torch.arange(b, device=dev)
        tl = target.long()
        orig = probs[idx, tl]
        full = eng.perturbed_forward(x, torch.ones(b, T, device=dev), "freeze")[idx, tl]     # mask.py:123-128
        scores = eng.blob_scores(x, target, self.max_mask_length, self.mask_type)
        sel = blob_select(scores, orig, full, T, self.max_mask_length, self.lam1, self.lam2, self.threshold)
        mask = blob_masks(sel["best"], T)
        k = blob_index(sel["best"], T)
        out["time_mask"] = mask
        out["freeze_score"] = score_at(scores, k)                                             # the loop-type score
        time_mask_outputs(eng, x, target, mask, out)
        out["blob"] = sel["best"]
        out["blob_objective"] = sel["objective"]
        out["blob_minimal"] = sel["minimal"]
        out["blob_scores"] = scores


    def st_grid(self, x):
        if self.mask_grid is not None:
            return tuple(int(v) for v in self.mask_grid)
        return max(1, round(x.shape[3] / 32)), max(1, round(x.shape[4] / 32))

    def _run_spacetime(self, x, target, probs, out, want_traj):
        """maskType 'spacetime': init_mask('central') rows broadcast over the grid, n_iter iterations of the spacetime
        loop; st_mask = sigmoid(raw) [b,T,gh,gw], time_mask = its spatial mean per frame, and from time_mask the
        reverse score, ranking and snapped mask with the code of the temporal search."""
        eng = self.engine
        b, T = x.shape[0], x.shape[2]
        dev = x.device
        idx = torch.arange(b, device=dev)
        gh, gw = self.st_grid(x)
        rows, info = init_masks_central(eng, x, target, probs[idx, target.long()], self.threshold, "freeze")
        out["init_mask"] = rows.clone()
        raw = rows.view(b, T, 1, 1).expand(b, T, gh, gw).contiguous()
        traj, _ = eng.st_search(x, target, raw, self.lam1, self.lam2, self.n_iter, (gh, gw), self.mask_sigma,
                                lam3=self.lam3, lr=self.lr, want_traj=True)
        S = torch.empty_like(raw)
        with torch.cuda.device(dev):
            L.check(L.lib().ivf_sigmoid(L.ptr(raw), L.ptr(S), raw.numel(), L.stream()))
        mean = frame_means(S)
        out["st_mask"] = S
        out["time_mask"] = mean
        out["freeze_score"] = traj[-1, :, 4] if self.n_iter > 0 else torch.full((b,), float("nan"), device=dev)
        time_mask_outputs(eng, x, target, mean, out)
        if want_traj:
            out["traj"] = traj

    def _run_stcombi(self, x, target, probs, out):
        """maskType 'stcombi': score every one-box mask, pick the argmin of the spacetime loss on the device; st_mask is
        the binary S of the best box, time_mask its spatial mean per frame (the call of _run_spacetime), and from
        time_mask the reverse score, ranking and snapped mask with the code of the temporal search."""
        eng = self.engine
        b, T = x.shape[0], x.shape[2]
        dev = x.device
        idx = torch.arange(b, device=dev)
        tl = target.long()
        grid = self.st_grid(x)
        orig = probs[idx, tl]
        full = eng.perturbed_forward(x, torch.ones(b, T, device=dev), "freeze")[idx, tl]     # mask.py:123-128
        scores = eng.box_scores(x, target, grid, self.mask_sigma, self.max_mask_length, self.max_box)
        sel = box_select(scores, orig, full, T, grid, self.max_mask_length, self.max_box, self.lam1, self.lam2, self.lam3,
                         self.threshold)
        S = box_masks(sel["best"], T, grid)
        mean = frame_means(S)
        out["st_mask"] = S
        out["time_mask"] = mean
        out["freeze_score"] = score_at(scores, sel["index"])
        time_mask_outputs(eng, x, target, mean, out)
        out["box"] = sel["best"]
        out["box_objective"] = sel["objective"]
        out["box_minimal"] = sel["minimal"]
        out["box_scores"] = scores
        out["box_drop"] = box_drop(scores, orig, T, grid, self.max_mask_length, self.max_box)


RECORD_INT_FIELDS = ("clip_id", "pred_class", "target")
RECORD_FLOAT_FIELDS = ("original_score_guess", "original_score_true", "freeze_score", "reverse_score")
RECORD_FIELDS = RECORD_INT_FIELDS + RECORD_FLOAT_FIELDS


def pack_records(clip_ids, res, T, with_cam=False):
    """Fixed-size per-clip record [b, 7+T (+ cam)] int32 for the all-gather: clip id,
    pred_class, target as integers; the four scores and sigma(mask)[T] as bit-cast float32.
    with_cam=True appends the clip's Grad-CAM map res["gradcam"] [T', h, w] (bit-cast float32, row-major) -- the
    optional payload of SURVEY.md 8e; at [16,224,224] that is 3.2 MB per clip, a few milliseconds of xGMI time per
    step of 32 clips per GPU against seconds of search.  Every rank must use the same map shape."""
    dev = res["pred_class"].device
    ints = [torch.as_tensor(clip_ids, device=dev).to(torch.int32)]
    ints += [res[k].to(torch.int32) for k in RECORD_INT_FIELDS[1:]]
    flt = torch.stack([res[k].float() for k in RECORD_FLOAT_FIELDS], dim=1)
    parts = [flt, res["time_mask"].float()]
    if with_cam:
        cam = res["gradcam"]
        parts.append(cam.float().reshape(cam.shape[0], -1))
    flt = torch.cat(parts, dim=1).contiguous()
    return torch.cat([torch.stack(ints, dim=1), flt.view(torch.int32)], dim=1).contiguous()


def unpack_record(row, T, cam_shape=None):
    """One gathered row -> dict; cam_shape = (T', h, w) when the rows carry Grad-CAM maps (pack_records(with_cam=True))."""
    row = row.detach().cpu().contiguous()
    ni = len(RECORD_INT_FIELDS)
    d = {k: int(row[i]) for i, k in enumerate(RECORD_INT_FIELDS)}
    f = row[ni:].view(torch.float32)
    for i, k in enumerate(RECORD_FLOAT_FIELDS):
        d[k] = float(f[i])
    nf = len(RECORD_FLOAT_FIELDS)
    d["time_mask"] = f[nf:nf + T].numpy().copy()
    if cam_shape is not None:
        n = int(np.prod(cam_shape))
        if f.numel() != nf + T + n:
            raise L.IvfError(f"record has {f.numel() - nf - T} map values, cam_shape {tuple(cam_shape)} needs {n}")
        d["gradcam"] = f[nf + T:].numpy().reshape(cam_shape).copy()
    return d
