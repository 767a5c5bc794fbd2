"""Host-side owner of one libivf_hip network plan (I3D or CLSTM_4).

Holds the two device arenas (weights, workspace) as torch tensors -- PyTorch is
the allocator, nothing more -- and exposes the plan's entry points with torch
tensors in/out.  Everything that computes is in csrc/*.hip.
"""
import ctypes
import math
import os
from ctypes import byref, c_char, c_int, c_void_p

import numpy as np
import torch

import ivf_arch as arch
import ivf_lib as L


# arithmetic of the Unit3D convolutions unless a caller overrides it (see include/ivf_hip.h)
DEFAULT_MATH = os.environ.get("IVF_MATH", "bf16x6")   # fp32-class: 3-way bf16 split, 6 MFMA passes
# per-layer kernel autotuning when weights are first loaded (IVF_AUTOTUNE=0: built-in heuristic)
AUTOTUNE = os.environ.get("IVF_AUTOTUNE", "1") != "0"


def _mode_id(mode):
    """perturbation type -> the C-ABI's mode id; anything else fails as the reference's
    perturb_sequence does (mask.py:57 returns an unset local)."""
    if mode == "freeze":
        return 0
    if mode == "reverse":
        return 1
    raise UnboundLocalError("local variable 'perturbed_input' referenced before assignment")


def default_st_grid(H, W):
    """spatial mask grid where none is given: one cell per 32 input pixels (7x7 at 224^2, 4x5 at 120x160)"""
    return max(1, round(H / 32)), max(1, round(W / 32))


def rise_thresh(p):
    """The integer threshold of the RISE mask hash, computed here and nowhere else: a cell is frozen iff
    its 32-bit hash < floor(p 2^32), 0 < p < 1 (a p below 2^-32 would freeze nothing and is refused as well)."""
    try:
        p = float(p)
    except (TypeError, ValueError):
        raise L.IvfError(f"p must be a number in (0, 1), got {p!r}")
    if not 0.0 < p < 1.0:
        raise L.IvfError(f"p must be in (0, 1), got {p}")
    thresh = int(math.floor(p * 4294967296.0))
    if thresh < 1:
        raise L.IvfError(f"p = {p} is below 2^-32: no cell would ever be frozen")
    return thresh


def _arena(nbytes, device):
    # torch's caching allocator returns >=512-byte aligned blocks
    t = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    assert t.data_ptr() % 256 == 0
    return t


class _Engine:
    """What the three backbones share: one libivf_hip plan `ivf_<_prefix>_*`, its two arenas and the entry points every
    plan has.  A subclass fills its config struct, calls `_create`, and loads its weights."""
    _prefix = None
    _has_mode = True        # the plan's search / perturbed_forward take the perturbation type (not the TF plan)

    def __init__(self, num_classes, clip_shape, max_batch, device):
        L.require_gpu()
        self.device = torch.device(device if device is not None else "cuda")
        C, T, H, W = clip_shape
        self.clip_shape = (C, T, H, W)
        self.max_batch = int(max_batch)
        self.K = int(num_classes)

    def _fn(self, name):
        return getattr(L.lib(), f"ivf_{self._prefix}_{name}")

    def _create(self, cfg):
        """cfg: the plan's config struct, geometry and class count filled in here; create -> arenas -> bind."""
        cfg.B, cfg.num_classes = self.max_batch, self.K
        cfg.C, cfg.T, cfg.H, cfg.W = self.clip_shape
        self.cfg = cfg
        self._h = c_void_p()
        L.check(self._fn("create")(byref(cfg), byref(self._h)))
        with torch.cuda.device(self.device):
            self._weights = _arena(self._fn("weights_bytes")(self._h), self.device)
            self._ws = _arena(self._fn("workspace_bytes")(self._h), self.device)
        L.check(self._fn("bind")(self._h, L.ptr(self._weights), L.ptr(self._ws)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and L is not None and getattr(L, "_lib", None) is not None:
            getattr(L._lib, f"ivf_{self._prefix}_destroy")(h)
            self._h = c_void_p()

    @property
    def workspace_bytes(self):
        return self._ws.numel()

    # -------------------------------------------------------------- helpers
    def _param(self, sd, key):
        """state_dict tensor `key` (reference key scheme, optional 'module.' prefix, numpy accepted) on the device."""
        for k in (key, "module." + key):
            if k in sd:
                v = sd[k]
                if isinstance(v, np.ndarray):
                    v = torch.from_numpy(v)
                return L.f32c(v.detach().to(self.device))
        raise KeyError(f"state_dict is missing '{key}'")

    def _clip(self, x, any_batch=False):
        L.require_gpu(x)
        x = L.f32c(x)
        if x.dim() != 5 or tuple(x.shape[1:]) != self.clip_shape:
            raise L.IvfError(f"clip batch must be [b,{','.join(map(str, self.clip_shape))}], got {tuple(x.shape)}")
        if x.shape[0] > self.max_batch and not any_batch:
            raise L.IvfError(f"batch {x.shape[0]} exceeds the plan's maximum {self.max_batch}")
        return x

    def _targets(self, target, b):
        t = torch.as_tensor(target, device=self.device).to(torch.int32).reshape(-1).contiguous()
        if t.numel() != b:
            raise L.IvfError(f"need {b} targets, got {t.numel()}")
        return t

    def _mode_args(self, mode):
        return (_mode_id(mode),) if self._has_mode else ()

    # -------------------------------------------------------------- entry points
    def forward(self, x, want_logits=False):
        x = self._clip(x)
        b = x.shape[0]
        probs = torch.empty(b, self.K, device=self.device)
        logits = torch.empty(b, self.K, device=self.device) if want_logits else None
        with torch.cuda.device(self.device):
            L.check(self._fn("forward")(self._h, L.ptr(x), b, L.ptr(logits), L.ptr(probs), L.stream()))
        return (probs, logits) if want_logits else probs

    def backward(self, b, target=None, dout=None, want_dx=True):
        """Backward-data of the last forward.  Returns (score [b] or None, dx NCTHW or None)."""
        C, T, H, W = self.clip_shape
        tgt = self._targets(target, b) if target is not None else None
        dout = L.f32c(dout) if dout is not None else None
        score = torch.empty(b, device=self.device) if tgt is not None else None
        dx = torch.empty(b, C, T, H, W, device=self.device) if want_dx else None
        with torch.cuda.device(self.device):
            L.check(self._fn("backward")(self._h, b, L.ptr(tgt), L.ptr(dout), L.ptr(score), L.ptr(dx), L.stream()))
        return score, dx

    def search(self, x, target, raw_mask, lam1, lam2, N, lr=0.2, betas=(0.9, 0.999), eps=1e-8,
               state=None, want_traj=True, mode="freeze"):
        """N iterations of the hot loop (smth:193-214) on b clips.  raw_mask [b,T] is
        updated in place; state = (exp_avg, exp_avg_sq, steps_done) continues a search;
        mode = the perturbation the loop optimises through (temporalMaskType, smth:121,202)."""
        x = self._clip(x)
        b = x.shape[0]
        T = self.clip_shape[1]
        tgt = self._targets(target, b)
        L.require_gpu(raw_mask)
        if raw_mask.dtype != torch.float32 or not raw_mask.is_contiguous() or tuple(raw_mask.shape) != (b, T):
            raise L.IvfError("raw_mask must be a contiguous float32 [b,T] tensor")
        if state is None:
            state = (torch.zeros_like(raw_mask), torch.zeros_like(raw_mask), 0)
        m, v, done = state
        traj = torch.empty(N, b, 4, device=self.device) if want_traj else None
        with torch.cuda.device(self.device):
            L.check(self._fn("search")(self._h, L.ptr(x), b, L.ptr(tgt), L.ptr(raw_mask), L.ptr(m), L.ptr(v),
                                       lam1, lam2, lr, betas[0], betas[1], eps, int(N), done + 1,
                                       *self._mode_args(mode), L.ptr(traj), L.stream()))
        return traj, (m, v, done + int(N))

    def perturbed_forward(self, x, mask, mode="freeze"):
        x = self._clip(x)
        b = x.shape[0]
        mask = L.f32c(mask.to(self.device))
        if tuple(mask.shape) != (b, self.clip_shape[1]):
            raise L.IvfError("mask must be [b,T]")
        probs = torch.empty(b, self.K, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self._fn("perturbed_forward")(self._h, L.ptr(x), b, L.ptr(mask), *self._mode_args(mode),
                                                  L.ptr(probs), L.stream()))
        return probs

    def blob_scores(self, x, target, max_len=None, mode="freeze"):
        """Exhaustive one-blob search grid (maskType 'combi', ivf_*_blob_scores): scores [b, n] of target[clip]
        under every one-blob binary mask, in the order of ivf_search.blob_candidates(T, max_len).  The whole grid of
        b clips in one C call (chunks of the plan's max_batch rows; b itself may exceed max_batch)."""
        x = self._clip(x, any_batch=True)
        b, T = x.shape[0], self.clip_shape[1]
        ml = T if max_len is None else int(max_len)
        n = L.lib().ivf_blob_count(T, ml)
        if n < 0:
            raise L.IvfError(L.lib().ivf_last_error().decode())
        tgt = self._targets(target, b)
        scores = torch.empty(b, n, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self._fn("blob_scores")(self._h, L.ptr(x), b, L.ptr(tgt), ml, _mode_id(mode), L.ptr(scores),
                                            L.stream()))
        return scores

    # -------------------------------------------------------------- spatio-temporal masks (extension)
    _has_st = True          # ivf_<prefix>_stsearch / _stperturbed_forward exist (not for the TF plan)

    def _st_axes(self, grid, sigma):
        """(gh, gw, sigma, A_H [H,gh], A_W [W,gw]) on the device: ivf_stmask_axis_weights, built once per (grid, sigma).
        sigma None -> 0.5 * H / gh input pixels."""
        if not self._has_st:
            raise L.IvfError("spatio-temporal masks are built for the I3D and CLSTM plans only")
        gh, gw = (int(v) for v in grid)
        H, W = self.clip_shape[2:]
        sigma = 0.5 * H / gh if sigma is None else float(sigma)
        cache = self.__dict__.setdefault("_st_axis_cache", {})
        key = (gh, gw, sigma)
        if key not in cache:
            mats = []
            for n_out, n_in in ((H, gh), (W, gw)):
                a = np.empty((n_out, max(n_in, 1)), dtype=np.float32)
                L.check(L.lib().ivf_stmask_axis_weights(n_out, n_in, sigma, a.ctypes.data_as(c_void_p)))
                mats.append(torch.from_numpy(a).to(self.device))
            cache[key] = tuple(mats)
        return (gh, gw, sigma) + cache[key]

    def st_expand(self, S, grid, sigma=None):
        """M [b,T,H,W] = A_H S A_W^T for S [b,T,gh,gw] in [0,1] (bilinear upsampling + Gaussian blur, one linear map)."""
        gh, gw, _, AH, AW = self._st_axes(grid, sigma)
        L.require_gpu(S)
        S = L.f32c(S)
        C, T, H, W = self.clip_shape
        if S.dim() != 4 or tuple(S.shape[1:]) != (T, gh, gw):
            raise L.IvfError(f"S must be [b,{T},{gh},{gw}], got {tuple(S.shape)}")
        b = S.shape[0]
        M = torch.empty(b, T, H, W, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().ivf_stmask_expand_fwd(L.ptr(S), L.ptr(AH), L.ptr(AW), L.ptr(M), b, T, gh, gw, H, W, L.stream()))
        return M

    def st_search(self, x, target, raw, lam1, lam2, N, grid, sigma=None, lam3=None, lr=0.2, betas=(0.9, 0.999), eps=1e-8,
                  state=None, want_traj=True):
        """N iterations of the spacetime loop on b clips: raw [b,T,gh,gw] is updated in place, the perturbation is the
        per-pixel freeze by M = st_expand(sigmoid(raw)).  Returns (traj [N,b,5] = (J, l1, tvt, tvs, score), state);
        lam3 (spatial TV) defaults to lam2."""
        gh, gw, _, AH, AW = self._st_axes(grid, sigma)
        x = self._clip(x)
        b = x.shape[0]
        C, T, H, W = self.clip_shape
        tgt = self._targets(target, b)
        L.require_gpu(raw)
        if raw.dtype != torch.float32 or not raw.is_contiguous() or tuple(raw.shape) != (b, T, gh, gw):
            raise L.IvfError(f"raw must be a contiguous float32 [b,{T},{gh},{gw}] tensor")
        if state is None:
            state = (torch.zeros_like(raw), torch.zeros_like(raw), 0)
        m, v, done = state
        nbytes = L.lib().ivf_stsearch_workspace_bytes(b, T, H, W, gh, gw)
        if nbytes == 0:
            raise L.IvfError(L.lib().ivf_last_error().decode())
        ws = self.__dict__.get("_st_ws")
        if ws is None or ws.numel() < nbytes:
            with torch.cuda.device(self.device):
                ws = self._st_ws = _arena(nbytes, self.device)
        traj = torch.empty(N, b, 5, device=self.device) if want_traj else None
        with torch.cuda.device(self.device):
            L.check(self._fn("stsearch")(self._h, L.ptr(x), b, L.ptr(tgt), L.ptr(raw), L.ptr(m), L.ptr(v), L.ptr(AH),
                                         L.ptr(AW), gh, gw, lam1, lam2, lam2 if lam3 is None else lam3, lr, betas[0],
                                         betas[1], eps, int(N), done + 1, L.ptr(traj), L.ptr(ws), L.stream()))
        return traj, (m, v, done + int(N))

    def st_freeze(self, x, M):
        """x [b,C,T,H,W] frozen per pixel by M [b,T,H,W] (values in [0,1]): the perturbed clips, NCTHW (ivf_stfreeze_fwd)."""
        L.require_gpu(x)
        x, M = L.f32c(x), L.f32c(M.to(x.device))
        b, C, T, H, W = x.shape
        if tuple(M.shape) != (b, T, H, W):
            raise L.IvfError(f"M must be [b,{T},{H},{W}]")
        p = torch.empty_like(x)
        with torch.cuda.device(x.device):
            L.check(L.lib().ivf_stfreeze_fwd(L.ptr(x), L.ptr(M), L.ptr(p), b, C, T, H * W, 0, L.stream()))
        return p

    def st_perturbed_forward(self, x, M):
        """probs [b,K] of x frozen per pixel by M [b,T,H,W] (values in [0,1])."""
        if not self._has_st:
            raise L.IvfError("spatio-temporal masks are built for the I3D and CLSTM plans only")
        x = self._clip(x)
        b = x.shape[0]
        C, T, H, W = self.clip_shape
        M = L.f32c(M.to(self.device))
        if tuple(M.shape) != (b, T, H, W):
            raise L.IvfError(f"M must be [b,{T},{H},{W}]")
        probs = torch.empty(b, self.K, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self._fn("stperturbed_forward")(self._h, L.ptr(x), b, L.ptr(M), L.ptr(probs), L.stream()))
        return probs

    def box_scores(self, x, target, grid, sigma=None, max_len=None, max_box=None):
        """Exhaustive one-box search grid (maskType 'stcombi', ivf_*_box_scores): scores [b, n] of target[clip] with the
        clip frozen per pixel by every one-box binary mask on `grid` (expanded as st_expand expands it), in the order of
        ivf_search.box_candidates(T, grid, max_len, max_box).  max_len defaults to T, max_box to the whole grid; b may
        exceed max_batch (chunks of the plan's max_batch rows)."""
        gh, gw, _, AH, AW = self._st_axes(grid, sigma)
        x = self._clip(x, any_batch=True)
        b, T = x.shape[0], self.clip_shape[1]
        ml = T if max_len is None else int(max_len)
        mh, mw = (gh, gw) if max_box is None else (int(v) for v in max_box)
        n = L.lib().ivf_box_count(T, ml, gh, gw, mh, mw)
        if n < 0:
            raise L.IvfError(L.lib().ivf_last_error().decode())
        tgt = self._targets(target, b)
        scores = torch.empty(b, n, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self._fn("box_scores")(self._h, L.ptr(x), b, L.ptr(tgt), L.ptr(AH), L.ptr(AW), gh, gw, ml, mh, mw,
                                           L.ptr(scores), L.stream()))
        return scores

    # -------------------------------------------------------------- Integrated Gradients (extension)
    _has_ig = True          # ivf_<prefix>_ig / _ig_path_scores exist (not for the TF plan)

    def _ig_args(self, x, baseline, base):
        """(base_kind, base tensor or None, base_value) of a baseline: 'frozen' (frame 0 of the row's own clip at every
        frame), 'constant' (base: one value, default 0.0 = black) or 'clip' (base: a [b,C,T,H,W] tensor)."""
        if not self._has_ig:
            raise L.IvfError("Integrated Gradients is built for the I3D and CLSTM plans only")
        if baseline == "frozen":
            if base is not None:
                raise L.IvfError("baseline 'frozen' takes no base")
            return 0, None, 0.0
        if baseline == "constant":
            return 1, None, 0.0 if base is None else float(base)
        if baseline == "clip":
            if base is None:
                raise L.IvfError("baseline 'clip' needs base, a [b,C,T,H,W] tensor")
            L.require_gpu(base)
            base = L.f32c(base)
            if tuple(base.shape) != tuple(x.shape):
                raise L.IvfError(f"base must be {tuple(x.shape)}, got {tuple(base.shape)}")
            return 2, base, 0.0
        raise L.IvfError(f"baseline must be 'frozen', 'constant' or 'clip', got {baseline!r}")

    def _ig_rule(self, steps, alpha, weights, need_weights=True):
        """(K, alpha [K], w [K]) on the device, built on the host in fp32.  Default: the midpoint rule,
        alpha_k = (2k+1)/(2K), w_k = 1/K.  need_weights=False (forward only): w is None unless given."""
        if alpha is None:
            K = int(steps)
            if K < 1:
                raise L.IvfError(f"steps must be >= 1, got {steps}")
            alpha = (2.0 * np.arange(K, dtype=np.float32) + np.float32(1.0)) / np.float32(2 * K)
            if weights is None:
                weights = np.full(K, np.float32(1.0) / np.float32(K), dtype=np.float32)
        alpha = np.ascontiguousarray(np.asarray(alpha, dtype=np.float32).reshape(-1))
        K = alpha.size
        if K < 1:
            raise L.IvfError("alpha must hold at least one node")
        if weights is None:
            if need_weights:
                raise L.IvfError("explicit alpha needs explicit weights")
            return K, torch.from_numpy(alpha).to(self.device), None
        weights = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
        if weights.size != K:
            raise L.IvfError(f"need {K} weights, got {weights.size}")
        return K, torch.from_numpy(alpha).to(self.device), torch.from_numpy(weights).to(self.device)

    def ig_path_scores(self, x, target, baseline="frozen", base=None, alpha=None, steps=32):
        """Scores [b,K] of target[clip] at the path points x0 + alpha[k] (x - x0) (ivf_*_ig_path_scores: forward only,
        chunks of the plan's max_batch rows; b may exceed max_batch).  alpha=[0] scores the baseline itself."""
        x = self._clip(x, any_batch=True)
        b = x.shape[0]
        kind, base, value = self._ig_args(x, baseline, base)
        K, a, _ = self._ig_rule(steps, alpha, None, need_weights=False)
        tgt = self._targets(target, b)
        scores = torch.empty(b, K, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self._fn("ig_path_scores")(self._h, L.ptr(x), b, L.ptr(tgt), kind, L.ptr(base), value, L.ptr(a), K,
                                               L.ptr(scores), L.stream()))
        return scores

    def ig(self, x, target, steps=32, baseline="frozen", base=None, alpha=None, weights=None):
        """Integrated Gradients of target[clip] on b clips (ivf_*_ig; b may exceed max_batch).  Returns a dict of
        device tensors: ig_map [b,T,H,W], ig_frames, ig_abs_frames [b,T], ig_total [b], path_scores [b,K], score_x,
        score_base [b] and ig_gap = ig_total - (score_x - score_base), the quadrature error to choose `steps` by.
        score_base is the forward-only entry at alpha = [0] (the baseline staged exactly), score_x the plan's
        ordinary forward."""
        x = self._clip(x, any_batch=True)
        b = x.shape[0]
        C, T, H, W = self.clip_shape
        base_arg = base
        kind, base, value = self._ig_args(x, baseline, base)
        K, a, w = self._ig_rule(steps, alpha, weights)
        tgt = self._targets(target, b)
        nbytes = L.lib().ivf_ig_workspace_bytes(b, C, T, H * W, K)
        if nbytes == 0:
            raise L.IvfError(L.lib().ivf_last_error().decode())
        ws = self.__dict__.get("_ig_ws")
        if ws is None or ws.numel() < nbytes:
            with torch.cuda.device(self.device):
                ws = self._ig_ws = _arena(nbytes, self.device)
        dev = self.device
        out = dict(ig_map=torch.empty(b, T, H, W, device=dev), ig_frames=torch.empty(b, T, device=dev),
                   ig_abs_frames=torch.empty(b, T, device=dev), ig_total=torch.empty(b, device=dev),
                   path_scores=torch.empty(b, K, device=dev))
        with torch.cuda.device(dev):
            L.check(self._fn("ig")(self._h, L.ptr(x), b, L.ptr(tgt), kind, L.ptr(base), value, L.ptr(a), L.ptr(w), K,
                                   L.ptr(out["ig_map"]), L.ptr(out["ig_frames"]), L.ptr(out["ig_abs_frames"]),
                                   L.ptr(out["ig_total"]), L.ptr(out["path_scores"]), L.ptr(ws), L.stream()))
        out["score_base"] = self.ig_path_scores(x, tgt, baseline, base_arg, alpha=[0.0])[:, 0]
        out["score_x"] = self._score_x(x, tgt)
        out["ig_gap"] = out["ig_total"] - (out["score_x"] - out["score_base"])
        return out

    def _score_x(self, x, tgt):
        """score [b] of tgt[clip] under the plan's ordinary forward, in chunks of max_batch clips"""
        idx = tgt.long().view(-1, 1)
        return torch.cat([self.forward(x[i:i + self.max_batch]).gather(1, idx[i:i + self.max_batch])
                          for i in range(0, x.shape[0], self.max_batch)])[:, 0].contiguous()

    def _grid3(self, grid, default, max_cells=None):
        """(gt, gh, gw) of a grid-mask call (RISE, Shapley, curves), checked; grid None -> default"""
        T = self.clip_shape[1]
        if grid is None:
            grid = default
        try:
            gt, gh, gw = (int(v) for v in grid)
        except (TypeError, ValueError):
            raise L.IvfError(f"grid must be (gt, gh, gw), got {grid!r}")
        sides = 1 <= gt <= T <= 64 and 1 <= gh <= 32 and 1 <= gw <= 32
        if max_cells is None and not sides:
            raise L.IvfError(f"grid {(gt, gh, gw)}: need 1 <= gt <= T = {T} <= 64 and 1 <= gh, gw <= 32")
        if max_cells is not None and not (sides and gt * gh * gw <= max_cells):
            raise L.IvfError(f"grid {(gt, gh, gw)}: need 1 <= gt <= T = {T} <= 64, 1 <= gh, gw <= 32 and at most "
                             f"{max_cells} cells")
        return gt, gh, gw

    # -------------------------------------------------------------- RISE random-mask saliency (extension)
    def _rise_args(self, n_masks, p, grid, sigma, seed):
        """(gt, gh, gw, n, seed, thresh, A_H, A_W) of a RISE call, checked; grid None -> (min(T, 8),) + the spatial
        grid of the spacetime search (one cell per 32 input pixels)."""
        if not self._has_st:
            raise L.IvfError("RISE is built for the I3D and CLSTM plans only")
        C, T, H, W = self.clip_shape
        gt, gh, gw = self._grid3(grid, (min(T, 8),) + default_st_grid(H, W))
        n, seed = int(n_masks), int(seed)
        if n < 1:
            raise L.IvfError(f"n_masks must be >= 1, got {n_masks}")
        if not 0 <= seed < 2 ** 32:
            raise L.IvfError(f"seed must be in [0, 2^32), got {seed}")
        thresh = rise_thresh(p)
        _, _, _, AH, AW = self._st_axes((gh, gw), sigma)
        return gt, gh, gw, n, seed, thresh, AH, AW

    def rise_masks(self, n_masks=1024, p=0.5, grid=None, seed=0, first=0):
        """The sampled masks themselves (ivf_rise_masks): S [n_masks,gt,gh,gw] in {0, 1} of masks first ..
        first + n_masks - 1, 1 = cell frozen.  The same for every clip."""
        gt, gh, gw, n, seed, thresh, _, _ = self._rise_args(n_masks, p, grid, None, seed)
        S = torch.empty(n, gt, gh, gw, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().ivf_rise_masks(seed, thresh, int(first), n, gt, gh, gw, L.ptr(S), L.stream()))
        return S

    def rise_scores(self, x, target, n_masks=1024, p=0.5, grid=None, sigma=None, seed=0):
        """Scores [b, n_masks] of target[clip] with the clip frozen per pixel by each random mask (expanded as st_expand
        expands it): ivf_*_rise_scores, forward only, chunks of the plan's max_batch rows; b may exceed max_batch."""
        gt, gh, gw, n, seed, thresh, AH, AW = self._rise_args(n_masks, p, grid, sigma, seed)
        x = self._clip(x, any_batch=True)
        b = x.shape[0]
        tgt = self._targets(target, b)
        scores = torch.empty(b, n, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self._fn("rise_scores")(self._h, L.ptr(x), b, L.ptr(tgt), L.ptr(AH), L.ptr(AW), gt, gh, gw, n, seed,
                                            thresh, L.ptr(scores), L.stream()))
        return scores

    def rise_reduce(self, scores, orig, p=0.5, grid=None, seed=0):
        """ivf_rise_reduce on scores [b,n] and orig [b]: (cells [b,gt,gh,gw], count int32, mean_drop [b])."""
        s = L.f32c(scores)
        L.require_gpu(s)
        b, n = s.shape
        gt, gh, gw, n, seed, thresh, _, _ = self._rise_args(n, p, grid, None, seed)
        orig = L.f32c(orig.reshape(b))
        cells = torch.empty(b, gt, gh, gw, device=s.device)
        count = torch.empty(b, gt, gh, gw, dtype=torch.int32, device=s.device)
        mean_drop = torch.empty(b, device=s.device)
        with torch.cuda.device(s.device):
            L.check(L.lib().ivf_rise_reduce(L.ptr(s), L.ptr(orig), b, n, seed, thresh, gt, gh, gw, L.ptr(cells),
                                            L.ptr(count), L.ptr(mean_drop), L.stream()))
        return cells, count, mean_drop

    def rise(self, x, target, n_masks=1024, p=0.5, grid=None, sigma=None, seed=0):
        """RISE (Petsiuk et al. 2018) of target[clip] on b clips, b may exceed max_batch: n_masks random masks on
        grid = (gt, gh, gw), each cell frozen with probability p, one forward per mask, a cell's importance = the mean
        of score_x - score over the masks that froze it.  Returns a dict of device tensors: rise_scores [b,n],
        rise_cells [b,gt,gh,gw] (NaN where no mask froze the cell), rise_count (int32), rise_mean_drop [b], score_x [b]
        (the plan's ordinary forward), rise_map [b,T,H,W] (the cells repeated over the frames of their temporal cell
        and expanded with st_expand) and rise_frames [b,T] (its grid's spatial mean per frame)."""
        gt, gh, gw, n, seed, thresh, AH, AW = self._rise_args(n_masks, p, grid, sigma, seed)
        x = self._clip(x, any_batch=True)
        b = x.shape[0]
        C, T, H, W = self.clip_shape
        tgt = self._targets(target, b)
        score_x = self._score_x(x, tgt)
        scores = self.rise_scores(x, tgt, n, p, (gt, gh, gw), sigma, seed)
        cells, count, mean_drop = self.rise_reduce(scores, score_x, p, (gt, gh, gw), seed)
        kt = (torch.arange(T, device=self.device) * gt) // T
        S = cells[:, kt].contiguous()                                   # [b,T,gh,gw]
        frames = torch.empty(b, T, device=self.device)
        ah, aw = torch.full((1, gh), 1.0 / gh, device=self.device), torch.full((1, gw), 1.0 / gw, device=self.device)
        with torch.cuda.device(self.device):                            # ivf_search.frame_means' uniform-row trick
            L.check(L.lib().ivf_stmask_expand_fwd(L.ptr(S), L.ptr(ah), L.ptr(aw), L.ptr(frames), b, T, gh, gw, 1, 1,
                                                  L.stream()))
        return dict(rise_scores=scores, rise_cells=cells, rise_count=count, rise_mean_drop=mean_drop, score_x=score_x,
                    rise_map=self.st_expand(S, (gh, gw), sigma), rise_frames=frames)

    # -------------------------------------------------------------- Score-CAM (extension)
    SCORECAM_WEIGHTS = {"increase": 0, "softmax": 1}
    SCORECAM_PERTURB = {"freeze": 0, "blank": 1}
    SCORECAM_MAX_SIDE, SCORECAM_MAX_CELLS = 32, 8192

    def _scorecam_feat(self, layer):
        """(name, (nc, gt, gh, gw), feat) of a Score-CAM target layer; feat(x) -> A [b,nc,gt,gh,gw] of at most max_batch
        clips.  Each backbone names its layers as its Grad-CAM does."""
        raise L.IvfError("Score-CAM is built for the I3D and CLSTM plans only")

    @staticmethod
    def _scorecam_kind(table, what, value):
        if value not in table:
            raise L.IvfError(f"Score-CAM {what} must be one of {', '.join(repr(k) for k in table)}, got {value!r}")
        return table[value]

    def _scorecam_layer(self, layer, channels):
        """(name, first, nc, gt, gh, gw, feat) of a call, checked against the limits of ivf_scorecam_stage"""
        name, (C, gt, gh, gw), feat = self._scorecam_feat(layer)
        T = self.clip_shape[1]
        if not (1 <= gt <= T <= 64 and gh <= self.SCORECAM_MAX_SIDE and gw <= self.SCORECAM_MAX_SIDE
                and gt * gh * gw <= self.SCORECAM_MAX_CELLS):
            raise L.IvfError(f"Score-CAM target {name}: its map {gt}x{gh}x{gw} exceeds the limits gt <= T = {T} <= 64, "
                             f"gh, gw <= {self.SCORECAM_MAX_SIDE} and gt gh gw <= {self.SCORECAM_MAX_CELLS}")
        first, nc = 0, C
        if channels is not None:
            try:
                first, nc = (int(v) for v in channels)
            except (TypeError, ValueError):
                raise L.IvfError(f"channels must be (first, count), got {channels!r}")
            if not (0 <= first and 1 <= nc and first + nc <= C):
                raise L.IvfError(f"channels {(first, nc)} outside the {C} channels of {name}")
        return name, first, nc, gt, gh, gw, feat

    def scorecam_planes(self, x, layer=None, channels=None):
        """The activations a Score-CAM call perturbs with and what ivf_scorecam_normalise makes of them: dict of A
        [b,nc,gt,gh,gw] (channel-major fp32 copies of the layer's activations under the plan's ordinary forward; with
        channels = (first, count) that window of them), lo, hi [b,nc], valid [b,nc] (int32) and the freeze planes F
        [b,nc,gt,gh,gw].  b may exceed max_batch."""
        _, first, nc, gt, gh, gw, feat = self._scorecam_layer(layer, channels)
        x = self._clip(x, any_batch=True)
        b = x.shape[0]
        A = torch.cat([feat(x[i:i + self.max_batch])[:, first:first + nc] for i in range(0, b, self.max_batch)])
        A = L.f32c(A)
        dev = self.device
        out = dict(A=A, lo=torch.empty(b, nc, device=dev), hi=torch.empty(b, nc, device=dev),
                   valid=torch.empty(b, nc, dtype=torch.int32, device=dev), F=torch.empty_like(A))
        with torch.cuda.device(dev):
            L.check(L.lib().ivf_scorecam_normalise(L.ptr(A), b, nc, gt * gh * gw, L.ptr(out["lo"]), L.ptr(out["hi"]),
                                                   L.ptr(out["valid"]), L.ptr(out["F"]), L.stream()))
        return out

    def scorecam_scores(self, x, target, F, sigma=None, perturb="freeze"):
        """Scores [b,nc+1] of target[clip] with the clip perturbed by each plane of F [b,nc,gt,gh,gw] (expanded as
        st_expand expands it), the last the baseline row: ivf_*_scorecam_scores, forward only, chunks of the plan's
        max_batch rows across clip boundaries; b may exceed max_batch."""
        mode = self._scorecam_kind(self.SCORECAM_PERTURB, "perturb", perturb)
        x = self._clip(x, any_batch=True)
        b = x.shape[0]
        L.require_gpu(F)
        F = L.f32c(F)
        if F.dim() != 5 or F.shape[0] != b:
            raise L.IvfError(f"F must be [{b},nc,gt,gh,gw], got {tuple(F.shape)}")
        nc, gt, gh, gw = F.shape[1:]
        _, _, _, AH, AW = self._st_axes((gh, gw), sigma)
        tgt = self._targets(target, b)
        scores = torch.empty(b, nc + 1, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self._fn("scorecam_scores")(self._h, L.ptr(x), b, L.ptr(tgt), L.ptr(AH), L.ptr(AW), gt, gh, gw, L.ptr(F),
                                                nc, mode, L.ptr(scores), L.stream()))
        return scores

    def scorecam_reduce(self, scores, A, valid, weights="increase"):
        """ivf_scorecam_reduce on scores [b,nc+1], A [b,nc,gt,gh,gw] and valid [b,nc]: (weights [b,nc], cam [b,gt,gh,gw])."""
        kind = self._scorecam_kind(self.SCORECAM_WEIGHTS, "weights", weights)
        L.require_gpu(scores, A, valid)
        s, A = L.f32c(scores), L.f32c(A)
        valid = valid.to(torch.int32).contiguous()
        b, nc, gt, gh, gw = A.shape
        if tuple(s.shape) != (b, nc + 1) or tuple(valid.shape) != (b, nc):
            raise L.IvfError(f"need scores [{b},{nc + 1}] and valid [{b},{nc}], got {tuple(s.shape)} and {tuple(valid.shape)}")
        w = torch.empty(b, nc, device=s.device)
        cam = torch.empty(b, gt, gh, gw, device=s.device)
        with torch.cuda.device(s.device):
            L.check(L.lib().ivf_scorecam_reduce(L.ptr(s), L.ptr(A), L.ptr(valid), b, nc, gt * gh * gw, kind, L.ptr(w),
                                                L.ptr(cam), L.stream()))
        return w, cam

    def scorecam(self, x, target, layer=None, weights="increase", perturb="freeze", sigma=None, channels=None,
                 per_frame=True, out_hw=None):
        """Score-CAM (Wang et al. 2020) of target[clip] on b clips, b may exceed max_batch: every channel of `layer`
        (named as the backbone's Grad-CAM names it; `channels` = (first, count) a window of them) is normalised to a
        freeze plane, expanded to the clip (`sigma` as st_expand) and applied as the per-pixel freeze ('freeze') or as a
        multiplicative mask on a zero baseline ('blank'); a channel's weight is its row's score above the baseline
        row's ('increase') or the softmax of those ('softmax'); the map is relu(sum_k w_k A_k), resized and normalised
        as the Grad-CAM of the same layer.  Returns a dict of device tensors: scorecam_map [b,frames,H,W], scorecam_cam
        [b,gt,gh,gw], scorecam_weights [b,nc], scorecam_scores [b,nc+1], scorecam_valid [b,nc], score_x [b] (the plan's
        ordinary forward) and score_base [b] (the baseline row)."""
        self._scorecam_kind(self.SCORECAM_WEIGHTS, "weights", weights)        # refuse before any forward
        self._scorecam_kind(self.SCORECAM_PERTURB, "perturb", perturb)
        x = self._clip(x, any_batch=True)
        b = x.shape[0]
        C, T, H, W = self.clip_shape
        oh, ow = out_hw if out_hw is not None else (H, W)
        tgt = self._targets(target, b)
        planes = self.scorecam_planes(x, layer, channels)
        gt, gh, gw = planes["A"].shape[2:]
        scores = self.scorecam_scores(x, tgt, planes["F"], sigma, perturb)
        w, cam = self.scorecam_reduce(scores, planes["A"], planes["valid"], weights)
        step = T // gt
        out = torch.empty(b, gt * step, oh, ow, device=self.device)
        mm = torch.empty(b, gt, 2, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().ivf_cam_resize_normalise(L.ptr(cam), L.ptr(out), L.ptr(mm), b, gt, gh, gw, int(oh), int(ow),
                                                     step, 1 if per_frame else 0, L.stream()))
        return dict(scorecam_map=out, scorecam_cam=cam, scorecam_weights=w, scorecam_scores=scores,
                    scorecam_valid=planes["valid"], score_x=self._score_x(x, tgt), score_base=scores[:, -1].contiguous())

    # -------------------------------------------------------------- SmoothGrad / SmoothGrad^2 / VarGrad (extension)
    def _sg_args(self, n_samples, level, seed):
        """(n, level, seed) of a SmoothGrad call, checked"""
        if not self._has_ig:
            raise L.IvfError("SmoothGrad is built for the I3D and CLSTM plans only")
        try:
            n, seed, level = int(n_samples), int(seed), float(level)
        except (TypeError, ValueError):
            raise L.IvfError(f"n_samples, level, seed must be numbers, got {n_samples!r}, {level!r}, {seed!r}")
        if not 1 <= n <= 2 ** 24:
            raise L.IvfError(f"n_samples must be in [1, 2^24], got {n_samples}")
        if not (math.isfinite(level) and level >= 0.0):
            raise L.IvfError(f"level must be finite and >= 0, got {level}")
        if not 0 <= seed < 2 ** 32:
            raise L.IvfError(f"seed must be in [0, 2^32), got {seed}")
        return n, level, seed

    def sg_noise(self, n_samples=32, seed=0, first=0):
        """The noise itself (ivf_sg_noise): z [n_samples,C,T,H,W] of samples first .. first + n_samples - 1, one standard
        normal per (seed, sample, element).  The same for every clip."""
        n, _, seed = self._sg_args(n_samples, 0.0, seed)
        C, T, H, W = self.clip_shape
        z = torch.empty(n, C, T, H, W, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().ivf_sg_noise(seed, int(first), n, C, T, H * W, L.ptr(z), L.stream()))
        return z

    def smoothgrad(self, x, target, n_samples=32, level=0.15, seed=0):
        """SmoothGrad (Smilkov et al. 2017), SmoothGrad^2 and VarGrad (Hooker et al. 2019) of target[clip] on b clips
        (ivf_*_smoothgrad; b may exceed max_batch): n_samples noisy copies x + sigma z_k of each clip, sigma = level *
        (max(x_clip) - min(x_clip)), one forward and backward each.  Returns a dict of device tensors: sg_map (sum over
        the channels of |mean gradient|), sq_map (of the mean squared gradient), var_map (of the unbiased variance of
        the gradient; 0 at n_samples = 1) [b,T,H,W], sg_frames, sq_frames, var_frames [b,T], sample_scores [b,n],
        sigma [b] and score_x [b] (the plan's ordinary forward).  n_samples = 1, level = 0 is plain gradient saliency."""
        n, level, seed = self._sg_args(n_samples, level, seed)
        x = self._clip(x, any_batch=True)
        b = x.shape[0]
        C, T, H, W = self.clip_shape
        tgt = self._targets(target, b)
        nbytes = L.lib().ivf_sg_workspace_bytes(b, C, T, H * W, n)
        if nbytes == 0:
            raise L.IvfError(L.lib().ivf_last_error().decode())
        ws = self.__dict__.get("_sg_ws")
        if ws is None or ws.numel() < nbytes:
            self._sg_ws = None
            with torch.cuda.device(self.device):
                ws = self._sg_ws = _arena(nbytes, self.device)
        dev = self.device
        out = dict(sg_map=torch.empty(b, T, H, W, device=dev), sq_map=torch.empty(b, T, H, W, device=dev),
                   var_map=torch.empty(b, T, H, W, device=dev), sg_frames=torch.empty(b, T, device=dev),
                   sq_frames=torch.empty(b, T, device=dev), var_frames=torch.empty(b, T, device=dev),
                   sample_scores=torch.empty(b, n, device=dev), sigma=torch.empty(b, device=dev))
        with torch.cuda.device(dev):
            L.check(self._fn("smoothgrad")(self._h, L.ptr(x), b, L.ptr(tgt), n, level, seed, L.ptr(out["sg_map"]),
                                           L.ptr(out["sq_map"]), L.ptr(out["var_map"]), L.ptr(out["sg_frames"]),
                                           L.ptr(out["sq_frames"]), L.ptr(out["var_frames"]),
                                           L.ptr(out["sample_scores"]), L.ptr(out["sigma"]), L.ptr(ws), L.stream()))
        out["score_x"] = self._score_x(x, tgt)
        return out

    # -------------------------------------------------------------- Shapley value sampling (extension)
    def _shap_args(self, n_perms, grid, sigma, seed, antithetic=True):
        """(gt, gh, gw, n, seed, antithetic, A_H, A_W) of a Shapley call, checked; grid None -> (T, 1, 1): the players
        are the frames."""
        if not self._has_st:
            raise L.IvfError("Shapley value sampling is built for the I3D and CLSTM plans only")
        gt, gh, gw = self._grid3(grid, (self.clip_shape[1], 1, 1), 4096)
        try:
            n, seed = int(n_perms), int(seed)
        except (TypeError, ValueError):
            raise L.IvfError(f"n_perms and seed must be integers, got {n_perms!r}, {seed!r}")
        if not 1 <= n <= 2 ** 20:
            raise L.IvfError(f"n_perms must be in [1, 2^20], got {n_perms}")
        if not 0 <= seed < 2 ** 32:
            raise L.IvfError(f"seed must be in [0, 2^32), got {seed}")
        _, _, _, AH, AW = self._st_axes((gh, gw), sigma)
        return gt, gh, gw, n, seed, int(bool(antithetic)), AH, AW

    def shap_ranks(self, n_perms=64, grid=None, seed=0, antithetic=True, first=0):
        """The sampled permutations themselves (ivf_shap_ranks): int16 [n_perms, gt gh gw] holding the uint16 rank
        (0 .. P-1) of every cell in permutations first .. first + n_perms - 1; cell c is frozen from prefix rank + 1
        on.  The same for every clip."""
        gt, gh, gw, n, seed, anti, _, _ = self._shap_args(n_perms, grid, None, seed, antithetic)
        ranks = torch.empty(n, gt * gh * gw, dtype=torch.int16, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().ivf_shap_ranks(seed, anti, int(first), n, gt, gh, gw, L.ptr(ranks), L.stream()))
        return ranks

    def shap_scores(self, x, target, n_perms=64, grid=None, sigma=None, seed=0, antithetic=True):
        """Scores [b, n_perms, P+1] of target[clip]: entry [.., k, j] has the j cells of lowest rank in permutation k
        frozen per pixel (expanded as st_expand expands a mask), so [.., 0] is the clip and [.., P] the fully frozen
        clip: ivf_*_shap_scores, forward only, chunks of the plan's max_batch rows; b may exceed max_batch."""
        gt, gh, gw, n, seed, anti, AH, AW = self._shap_args(n_perms, grid, sigma, seed, antithetic)
        x = self._clip(x, any_batch=True)
        b = x.shape[0]
        tgt = self._targets(target, b)
        ranks = self.shap_ranks(n, (gt, gh, gw), seed, anti)
        scores = torch.empty(b, n, gt * gh * gw + 1, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self._fn("shap_scores")(self._h, L.ptr(x), b, L.ptr(tgt), L.ptr(AH), L.ptr(AW), gt, gh, gw, n,
                                            L.ptr(ranks), L.ptr(scores), L.stream()))
        return scores

    def shap_reduce(self, scores, grid=None, seed=0, antithetic=True):
        """ivf_shap_reduce on scores [b,n,P+1] with the rank table of (grid, seed, antithetic): (cells [b,gt,gh,gw],
        stderr, count int32, total [b])."""
        s = L.f32c(scores)
        L.require_gpu(s)
        if s.dim() != 3:
            raise L.IvfError(f"scores must be [b, n_perms, P+1], got {tuple(s.shape)}")
        b, n, rows = s.shape
        gt, gh, gw, n, seed, anti, _, _ = self._shap_args(n, grid, None, seed, antithetic)
        if rows != gt * gh * gw + 1:
            raise L.IvfError(f"scores {tuple(s.shape)} do not hold the {gt * gh * gw + 1} prefixes of grid {(gt, gh, gw)}")
        ranks = self.shap_ranks(n, (gt, gh, gw), seed, anti)
        cells = torch.empty(b, gt, gh, gw, device=s.device)
        stderr = torch.empty(b, gt, gh, gw, device=s.device)
        count = torch.empty(b, gt, gh, gw, dtype=torch.int32, device=s.device)
        total = torch.empty(b, device=s.device)
        with torch.cuda.device(s.device):
            L.check(L.lib().ivf_shap_reduce(L.ptr(s), L.ptr(ranks), b, n, gt, gh, gw, L.ptr(cells), L.ptr(stderr),
                                            L.ptr(count), L.ptr(total), L.stream()))
        return cells, stderr, count, total

    def shapley(self, x, target, n_perms=64, grid=None, sigma=None, seed=0, antithetic=True):
        """Shapley values of the cells of grid = (gt, gh, gw) (default (T, 1, 1): the frames) under the per-pixel
        freeze, by permutation sampling (Castro et al. 2009), for target[clip] on b clips, b may exceed max_batch:
        along each of n_perms permutations the cells are frozen one after another, one forward per prefix (n_perms (P+1)
        rows a clip); a cell's value is the mean score drop on its entry, > 0 where freezing it lowers the score.
        antithetic: every odd permutation is the one before it reversed.  Returns a dict of device tensors: shap_scores
        [b,n,P+1], shap_cells, shap_stderr (the standard error of the mean), shap_count (int32) [b,gt,gh,gw], shap_total
        [b] (= mean of score(clip) - score(fully frozen clip), what the cells sum to), score_x [b] (the plan's ordinary
        forward), shap_map [b,T,H,W] (the cells repeated over the frames of their temporal cell and expanded with
        st_expand) and shap_frames [b,T] (a temporal cell's spatial sum shared equally among its frames: it sums to
        the sum of the cells)."""
        gt, gh, gw, n, seed, anti, AH, AW = self._shap_args(n_perms, grid, sigma, seed, antithetic)
        x = self._clip(x, any_batch=True)
        b = x.shape[0]
        tgt = self._targets(target, b)
        score_x = self._score_x(x, tgt)
        scores = self.shap_scores(x, tgt, n, (gt, gh, gw), sigma, seed, anti)
        cells, stderr, count, total = self.shap_reduce(scores, (gt, gh, gw), seed, anti)
        amap, frames = self._cell_maps(cells, gt, gh, gw, sigma)
        return dict(shap_scores=scores, shap_cells=cells, shap_stderr=stderr, shap_count=count, shap_total=total,
                    score_x=score_x, shap_map=amap, shap_frames=frames)

    def _cell_maps(self, cells, gt, gh, gw, sigma):
        """(map [b,T,H,W], frames [b,T]) of additive cell values [b,gt,gh,gw] (Shapley, KernelSHAP, LIME): the cells
        repeated over the frames of their temporal cell and expanded with st_expand; a temporal cell's spatial sum
        shared equally among its frames, so that the frames sum to the cells"""
        b, T = cells.shape[0], self.clip_shape[1]
        kt = (torch.arange(T, device=self.device) * gt) // T
        S = cells[:, kt].contiguous()                                   # [b,T,gh,gw]
        share = 1.0 / torch.bincount(kt, minlength=gt).to(torch.float32)[kt]            # 1 / frames of the frame's cell
        frames = torch.empty(b, T, device=self.device)
        ah, aw = torch.ones(1, gh, device=self.device), torch.ones(1, gw, device=self.device)
        with torch.cuda.device(self.device):                            # unit rows: the spatial sum per frame
            L.check(L.lib().ivf_stmask_expand_fwd(L.ptr(S), L.ptr(ah), L.ptr(aw), L.ptr(frames), b, T, gh, gw, 1, 1,
                                                  L.stream()))
        return self.st_expand(S, (gh, gw), sigma), frames * share

    # -------------------------------------------------------------- KernelSHAP and LIME (extension)
    LIN_MAX_PLAYERS, LIN_MAX_ROWS = 1024, 2 ** 20

    def _lin_args(self, n_samples, grid, sigma, seed):
        """(gt, gh, gw, n, seed, A_H, A_W) of a linear-surrogate call, checked; grid None -> (T, 1, 1): the players are
        the frames."""
        if not self._has_st:
            raise L.IvfError("KernelSHAP and LIME are built for the I3D and CLSTM plans only")
        gt, gh, gw = self._grid3(grid, (self.clip_shape[1], 1, 1), self.LIN_MAX_PLAYERS)
        if gt * gh * gw < 2:
            raise L.IvfError(f"grid {(gt, gh, gw)}: a linear surrogate needs at least 2 cells")
        try:
            n, seed = int(n_samples), int(seed)
        except (TypeError, ValueError):
            raise L.IvfError(f"n_samples and seed must be integers, got {n_samples!r}, {seed!r}")
        if not 1 <= n <= self.LIN_MAX_ROWS:
            raise L.IvfError(f"n_samples must be in [1, 2^20], got {n_samples}")
        if not 0 <= seed < 2 ** 32:
            raise L.IvfError(f"seed must be in [0, 2^32), got {seed}")
        _, _, _, AH, AW = self._st_axes((gh, gw), sigma)
        return gt, gh, gw, n, seed, AH, AW

    @staticmethod
    def kshap_size_table(P):
        """The integer table KernelSHAP's coalition sizes are drawn with, computed here and nowhere else:
        uint32 [P-2], floor(2^32 CDF(i)) for i = 1 .. P-2, the CDF that of q(s) ~ 1 / (s (P-s)) on 1 .. P-1 (the
        Shapley kernel summed over the coalitions of a size), by an fp64 cumsum."""
        s = np.arange(1, P, dtype=np.float64)
        c = np.cumsum(1.0 / (s * (P - s)))
        return np.floor(4294967296.0 * (c[:P - 2] / c[-1])).astype(np.uint32)

    @staticmethod
    def lime_weight_table(P, width=0.25):
        """fp64 [P+1]: LIME's sample weight by the number m of frozen cells, exp(-D^2 / (2 width^2)) with
        D = 1 - sqrt((P - m) / P): lime_image's cosine distance to the unperturbed clip under its exponential kernel."""
        m = np.arange(P + 1, dtype=np.float64)
        D = 1.0 - np.sqrt((P - m) / P)
        return np.exp(-(D * D) / (2.0 * width * width))

    def _lin_check_kshap(self, n, P, paired):
        if n < P - 1:
            raise L.IvfError(f"KernelSHAP needs n_samples >= P - 1 = {P - 1} rows (got {n}): fewer leave the system singular")
        if paired and n % 2:
            raise L.IvfError(f"paired KernelSHAP rows come two by two: n_samples must be even, got {n}")

    def kshap_rows(self, n_samples=256, grid=None, seed=0, paired=True, first=0):
        """The sampled KernelSHAP rows themselves (ivf_kshap_rows): (bits int32 [n, ceil(P/32)] holding the uint32
        words -- bit c % 32 of word c / 32 set: the row freezes cell c --, sizes int16 [n]) of rows first ..
        first + n_samples - 1.  The same for every clip."""
        gt, gh, gw, n, seed, _, _ = self._lin_args(n_samples, grid, None, seed)
        P = gt * gh * gw
        # one spare word: at P = 2 the table is empty and the tensor would have no address
        table = torch.from_numpy(np.concatenate([self.kshap_size_table(P), np.zeros(1, np.uint32)]).view(np.int32))
        table = table.to(self.device)
        bits = torch.empty(n, (P + 31) // 32, dtype=torch.int32, device=self.device)
        sizes = torch.empty(n, dtype=torch.int16, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().ivf_kshap_rows(seed, int(bool(paired)), int(first), n, gt, gh, gw, L.ptr(table), L.ptr(bits),
                                           L.ptr(sizes), L.stream()))
        return bits, sizes

    def lime_rows(self, n_samples=1024, p=0.5, grid=None, seed=0, first=0):
        """The sampled LIME rows themselves (ivf_lime_rows), packed as kshap_rows packs them: the bits of
        rise_masks(n_samples, p, grid, seed)."""
        gt, gh, gw, n, seed, _, _ = self._lin_args(n_samples, grid, None, seed)
        bits = torch.empty(n, (gt * gh * gw + 31) // 32, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().ivf_lime_rows(seed, rise_thresh(p), int(first), n, gt, gh, gw, L.ptr(bits), L.stream()))
        return bits

    def _lin_bits(self, bits, P):
        if not torch.is_tensor(bits) or bits.dtype != torch.int32 or bits.dim() != 2 or \
                bits.shape[1] != (P + 31) // 32 or bits.shape[0] < 1 or not bits.is_contiguous():
            raise L.IvfError(f"bits must be a contiguous int32 [n, {(P + 31) // 32}] tensor (kshap_rows, lime_rows), got "
                             f"{getattr(bits, 'dtype', type(bits))} {tuple(getattr(bits, 'shape', ()))}")
        L.require_gpu(bits)
        return bits

    def lin_scores(self, x, target, bits, grid=None, sigma=None):
        """Scores [b, n+1] of target[clip]: entry [.., k] has the cells of row k of bits frozen per pixel (expanded as
        st_expand expands a mask), entry [.., n] every cell: ivf_*_lin_scores, forward only, chunks of the plan's
        max_batch rows; b may exceed max_batch."""
        if not torch.is_tensor(bits) or bits.dim() != 2:
            raise L.IvfError("bits must be an int32 [n, ceil(P/32)] tensor (kshap_rows, lime_rows)")
        gt, gh, gw, n, _, AH, AW = self._lin_args(bits.shape[0], grid, sigma, 0)
        bits = self._lin_bits(bits, gt * gh * gw)
        x = self._clip(x, any_batch=True)
        b = x.shape[0]
        tgt = self._targets(target, b)
        scores = torch.empty(b, n + 1, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self._fn("lin_scores")(self._h, L.ptr(x), b, L.ptr(tgt), L.ptr(AH), L.ptr(AW), gt, gh, gw, n,
                                           L.ptr(bits), L.ptr(scores), L.stream()))
        return scores

    LIN_KINDS = {"kernelshap": 0, "lime": 1}

    def lin_solve(self, kind, scores, score_x, bits, P, wtab=None, ridge=0.0):
        """The fit of scores [b,n+1] and score_x [b] on the rows `bits` of P players, fp64 on the device
        (ivf_lin_moments -> ivf_lin_solve -> ivf_lin_fit): kind 'kernelshap' (unit weights, the efficiency constraint
        solved exactly) or 'lime' (wtab [P+1] fp64 by the number of frozen cells, ridge, a free intercept).  Returns a
        dict of device tensors: cells [b,P], intercept [b], total [b] (score_x - the fully frozen row's score), ok
        (int32 [b]: 0 where a score of the clip is not finite, and everywhere where the system is singular; then the
        clip's cells, intercept and r2 are NaN) and r2 [b]."""
        if kind not in self.LIN_KINDS:
            raise L.IvfError(f"kind must be one of {', '.join(repr(k) for k in self.LIN_KINDS)}, got {kind!r}")
        P = int(P)
        if not 1 <= P <= self.LIN_MAX_PLAYERS:
            raise L.IvfError(f"need 1 <= P <= {self.LIN_MAX_PLAYERS} players, got {P}")
        bits = self._lin_bits(bits, P)
        n = bits.shape[0]
        s = L.f32c(scores)
        L.require_gpu(s)
        if s.dim() != 2 or s.shape[1] != n + 1:
            raise L.IvfError(f"scores must be [b, {n + 1}] (the {n} rows and the fully frozen one), got {tuple(s.shape)}")
        b = s.shape[0]
        sx = L.f32c(score_x.reshape(b))
        dev = s.device
        wt = None
        if wtab is not None:
            wt = torch.as_tensor(np.ascontiguousarray(np.asarray(wtab, np.float64).reshape(-1))).to(dev)
            if wt.numel() != P + 1:
                raise L.IvfError(f"wtab must hold P + 1 = {P + 1} weights, got {wt.numel()}")
        f64 = dict(dtype=torch.float64, device=dev)
        N, v, Wsum = torch.empty(P, P, **f64), torch.empty(P, **f64), torch.empty(1, **f64)
        r, t, wrow = torch.empty(b, P, **f64), torch.empty(b, **f64), torch.empty(n, **f64)
        ok = torch.empty(b, dtype=torch.int32, device=dev)
        cells, icpt, total, r2 = (torch.empty(b, P, device=dev), torch.empty(b, device=dev), torch.empty(b, device=dev),
                                  torch.empty(b, device=dev))
        work = _arena(L.lib().ivf_lin_workspace_bytes(P), dev)
        with torch.cuda.device(dev):
            L.check(L.lib().ivf_lin_moments(L.ptr(s), L.ptr(sx), L.ptr(bits), L.ptr(wt), b, n, P, L.ptr(N), L.ptr(v),
                                            L.ptr(Wsum), L.ptr(r), L.ptr(t), L.ptr(wrow), L.ptr(ok), L.stream()))
            L.check(L.lib().ivf_lin_solve(self.LIN_KINDS[kind], L.ptr(N), L.ptr(v), L.ptr(Wsum), L.ptr(r), L.ptr(t),
                                          L.ptr(s), L.ptr(sx), b, n, P, float(ridge), L.ptr(work), L.ptr(cells),
                                          L.ptr(icpt), L.ptr(total), L.ptr(ok), L.stream()))
            L.check(L.lib().ivf_lin_fit(L.ptr(s), L.ptr(sx), L.ptr(bits), L.ptr(wrow), L.ptr(cells), L.ptr(icpt), L.ptr(t),
                                        L.ptr(Wsum), L.ptr(ok), b, n, P, L.ptr(r2), L.stream()))
        return dict(cells=cells, intercept=icpt, total=total, ok=ok, r2=r2)

    def kernelshap(self, x, target, n_samples=256, grid=None, sigma=None, seed=0, paired=True):
        """KernelSHAP (Lundberg & Lee 2017) of the cells of grid = (gt, gh, gw) (default (T, 1, 1): the frames) under
        the per-pixel freeze, for target[clip] on b clips, b may exceed max_batch: n_samples coalitions whose sizes
        follow the Shapley kernel (paired: every odd row is the complement of the one before it), one forward each and
        one for the fully frozen clip, then the least-squares fit of the score drops under the efficiency constraint,
        in fp64 on the device.  A cell's value is > 0 where freezing it lowers the score.  Returns a dict of device
        tensors: kshap_scores [b,n+1], kshap_cells [b,gt,gh,gw], kshap_total [b] (= score_x - score(fully frozen
        clip), what the cells sum to), kshap_ok (int32 [b]; 0: a score was not finite or the sampled system is singular,
        the cells are NaN), kshap_r2 [b], kshap_sizes (int16 [n]), score_x [b], kshap_map [b,T,H,W] and kshap_frames
        [b,T] (built from the cells as shapley() builds its own)."""
        gt, gh, gw, n, seed, AH, AW = self._lin_args(n_samples, grid, sigma, seed)
        P = gt * gh * gw
        self._lin_check_kshap(n, P, paired)
        x = self._clip(x, any_batch=True)
        b = x.shape[0]
        tgt = self._targets(target, b)
        score_x = self._score_x(x, tgt)
        bits, sizes = self.kshap_rows(n, (gt, gh, gw), seed, paired)
        scores = self.lin_scores(x, tgt, bits, (gt, gh, gw), sigma)
        fit = self.lin_solve("kernelshap", scores, score_x, bits, P)
        cells = fit["cells"].reshape(b, gt, gh, gw)
        amap, frames = self._cell_maps(cells, gt, gh, gw, sigma)
        return dict(kshap_scores=scores, kshap_cells=cells, kshap_total=fit["total"], kshap_ok=fit["ok"],
                    kshap_r2=fit["r2"], kshap_sizes=sizes, score_x=score_x, kshap_map=amap, kshap_frames=frames)

    def lime(self, x, target, n_samples=1024, p=0.5, grid=None, sigma=None, seed=0, width=0.25, ridge=1.0):
        """LIME (Ribeiro et al. 2016) of the cells of grid = (gt, gh, gw) (default (T, 1, 1): the frames) under the
        per-pixel freeze, for target[clip] on b clips, b may exceed max_batch: n_samples Bernoulli(p) rows (RISE's
        masks), one forward each, then the ridge regression of the score drops on the frozen cells with a free
        intercept, every row weighted by exp(-D^2 / (2 width^2)) of its distance D to the clip, in fp64 on the device.
        Returns a dict of device tensors: lime_scores [b,n+1] (entry n: the fully frozen clip, not part of the fit),
        lime_cells [b,gt,gh,gw], lime_intercept [b], lime_ok (int32 [b]), lime_r2 [b], score_x [b], lime_map [b,T,H,W]
        and lime_frames [b,T]."""
        gt, gh, gw, n, seed, AH, AW = self._lin_args(n_samples, grid, sigma, seed)
        P = gt * gh * gw
        try:
            width, ridge = float(width), float(ridge)
        except (TypeError, ValueError):
            raise L.IvfError(f"width and ridge must be numbers, got {width!r}, {ridge!r}")
        if not (width > 0.0 and math.isfinite(width)):
            raise L.IvfError(f"width must be a finite number > 0, got {width}")
        if not (ridge >= 0.0 and math.isfinite(ridge)):
            raise L.IvfError(f"ridge must be a finite number >= 0, got {ridge}")
        x = self._clip(x, any_batch=True)
        b = x.shape[0]
        tgt = self._targets(target, b)
        score_x = self._score_x(x, tgt)
        bits = self.lime_rows(n, p, (gt, gh, gw), seed)
        scores = self.lin_scores(x, tgt, bits, (gt, gh, gw), sigma)
        fit = self.lin_solve("lime", scores, score_x, bits, P, self.lime_weight_table(P, width), ridge)
        cells = fit["cells"].reshape(b, gt, gh, gw)
        amap, frames = self._cell_maps(cells, gt, gh, gw, sigma)
        return dict(lime_scores=scores, lime_cells=cells, lime_intercept=fit["intercept"], lime_ok=fit["ok"],
                    lime_r2=fit["r2"], score_x=score_x, lime_map=amap, lime_frames=frames)

    # -------------------------------------------------------------- deletion / insertion curves (extension)
    def _curve_args(self, grid, sigma, step=1, curves=3, order=0):
        """(gt, gh, gw, step, curves, order, A_H, A_W) of a curve call, checked; grid None -> (T, 1, 1): the frames."""
        if not self._has_st:
            raise L.IvfError("deletion / insertion curves are built for the I3D and CLSTM plans only")
        gt, gh, gw = self._grid3(grid, (self.clip_shape[1], 1, 1), 4096)
        try:
            step, curves = int(step), int(curves)
        except (TypeError, ValueError):
            raise L.IvfError(f"step and curves must be integers, got {step!r}, {curves!r}")
        if not 1 <= step <= gt * gh * gw:
            raise L.IvfError(f"step must be in [1, {gt * gh * gw}] cells, got {step}")
        if curves not in (1, 2, 3):
            raise L.IvfError(f"curves must be 1 (deletion), 2 (insertion) or 3 (both), got {curves}")
        orders = {"morf": 0, "lerf": 1, 0: 0, 1: 1}
        if isinstance(order, (list, dict, set)) or order not in orders:
            raise L.IvfError(f"order must be 'morf' (most relevant first) or 'lerf', got {order!r}")
        _, _, _, AH, AW = self._st_axes((gh, gw), sigma)
        return gt, gh, gw, step, curves, orders[order], AH, AW

    def _curve_den(self, gh, gw, sigma):
        """The footprint weights sum_y A_H[y,i] sum_x A_W[x,j] of the pooling, fp64 on the host, stored as fp32 [gh,gw]"""
        _, _, sigma, AH, AW = self._st_axes((gh, gw), sigma)
        cache = self.__dict__.setdefault("_curve_den_cache", {})
        key = (gh, gw, sigma)
        if key not in cache:
            den = AH.cpu().numpy().astype(np.float64).sum(axis=0)[:, None] * AW.cpu().numpy().astype(np.float64).sum(axis=0)
            cache[key] = torch.from_numpy(den.astype(np.float32)).to(self.device)
        return cache[key]

    def curve_cells(self, attr, grid=None, sigma=None):
        """An attribution (higher = more important) as cells [b,t_in,gh,gw], t_in = gt or T.  attr per clip: [T] (the
        grid must then have gh = gw = 1), [gt,gh,gw], [T,gh,gw], or a pixel map [T,H,W], which is pooled per frame to
        the footprint-weighted mean sum_yx A_H[y,i] A_W[x,j] a[u,y,x] / (sum_y A_H[y,i] sum_x A_W[x,j]): the numerator
        by ivf_stmask_expand_bwd, the denominator fp64 on the host rounded once."""
        gt, gh, gw, _, _, _, AH, AW = self._curve_args(grid, sigma)
        C, T, H, W = self.clip_shape
        L.require_gpu(attr)
        a = L.f32c(attr)
        shape = tuple(a.shape[1:])
        if a.dim() == 2 and shape == (T,):
            if gh != 1 or gw != 1:
                raise L.IvfError(f"a frame profile [b,{T}] ranks frames only: grid {(gt, gh, gw)} needs a map")
            return a.view(-1, T, 1, 1)
        if a.dim() == 4 and shape in ((gt, gh, gw), (T, gh, gw)):
            return a
        if a.dim() == 4 and shape == (T, H, W):
            b = a.shape[0]
            num = torch.empty(b, T, gh, gw, device=self.device)
            with torch.cuda.device(self.device):
                L.check(L.lib().ivf_stmask_expand_bwd(L.ptr(a), L.ptr(AH), L.ptr(AW), L.ptr(num), b, T, gh, gw, H, W,
                                                      L.stream()))
            return num / self._curve_den(gh, gw, sigma)
        raise L.IvfError(f"attribution must be [b,{T}], [b,{gt},{gh},{gw}], [b,{T},{gh},{gw}] or [b,{T},{H},{W}], "
                         f"got {tuple(a.shape)}")

    def curve_ranks(self, attr, grid=None, sigma=None, order="morf"):
        """Per-clip rank table int16 [b, gt gh gw] (holding uint16 0 .. P-1) of an attribution (curve_cells shapes):
        ivf_curve_ranks.  order 'morf': rank = the number of cells with a higher value, ties to the lower index;
        'lerf' the reverse; NaN cells last either way."""
        gt, gh, gw, _, _, order, _, _ = self._curve_args(grid, sigma, order=order)
        cells = self.curve_cells(attr, (gt, gh, gw), sigma)
        b, t_in = cells.shape[:2]
        ranks = torch.empty(b, gt * gh * gw, dtype=torch.int16, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().ivf_curve_ranks(L.ptr(cells), b, t_in, self.clip_shape[1], gt, gh, gw, order, L.ptr(ranks),
                                            L.stream()))
        return ranks

    def curve_scores(self, x, target, ranks, grid=None, sigma=None, step=1, curves=3):
        """Scores [b, ncurves, J+1] of target[clip], J = ceil(P / step): deletion row j has the cells of rank below
        min(j step, P) frozen per pixel, insertion row j the others; ranks [b,P] is each clip's own table.
        ivf_*_curve_scores, forward only, chunks of the plan's max_batch rows across clips and curves; b may exceed
        max_batch."""
        gt, gh, gw, step, curves, _, AH, AW = self._curve_args(grid, sigma, step, curves)
        x = self._clip(x, any_batch=True)
        b, P = x.shape[0], gt * gh * gw
        tgt = self._targets(target, b)
        L.require_gpu(ranks)
        if ranks.dtype != torch.int16 or tuple(ranks.shape) != (b, P):
            raise L.IvfError(f"ranks must be an int16 [{b},{P}] tensor, got {ranks.dtype} {tuple(ranks.shape)}")
        ranks = ranks.contiguous()
        scores = torch.empty(b, 2 if curves == 3 else 1, -(-P // step) + 1, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self._fn("curve_scores")(self._h, L.ptr(x), b, L.ptr(tgt), L.ptr(AH), L.ptr(AW), gt, gh, gw,
                                             L.ptr(ranks), curves, step, L.ptr(scores), L.stream()))
        return scores

    def curve_reduce(self, scores, grid=None, step=1, curves=3):
        """ivf_curve_reduce on scores [b,ncurves,J+1]: (auc, auc_norm) [b,ncurves]; the trapezoid over the fraction of
        cells, and it rescaled so that the fully frozen clip is 0 and the clip 1 (NaN where the two scores are equal)."""
        gt, gh, gw, step, curves, _, _, _ = self._curve_args(grid, 0.0, step, curves)
        s = L.f32c(scores)
        L.require_gpu(s)
        P = gt * gh * gw
        want = (2 if curves == 3 else 1, -(-P // step) + 1)
        if s.dim() != 3 or tuple(s.shape[1:]) != want:
            raise L.IvfError(f"scores must be [b,{want[0]},{want[1]}] for grid {(gt, gh, gw)}, step {step}, curves "
                             f"{curves}; got {tuple(s.shape)}")
        b = s.shape[0]
        auc, norm = torch.empty(b, want[0], device=s.device), torch.empty(b, want[0], device=s.device)
        with torch.cuda.device(s.device):
            L.check(L.lib().ivf_curve_reduce(L.ptr(s), b, want[0], curves, P, step, L.ptr(auc), L.ptr(norm), L.stream()))
        return auc, norm

    def curve_random_baseline(self, shap_scores):
        """The expected curves of a random ranking from Shapley rows [b,n,P+1] of the same grid and sigma: [b,2,P+1] =
        (mean_k s[k][j], mean_k s[k][P-j]), deletion then insertion, ready for curve_reduce at step 1."""
        if not self._has_st:
            raise L.IvfError("deletion / insertion curves are built for the I3D and CLSTM plans only")
        s = L.f32c(shap_scores)
        if s.dim() != 3:
            raise L.IvfError(f"shap_scores must be [b, n_perms, P+1], got {tuple(s.shape)}")
        m = s.mean(dim=1)
        return torch.stack([m, m.flip(-1)], dim=1).contiguous()

    def faithfulness(self, x, target, attr, grid=None, sigma=None, step=1, order="morf"):
        """Deletion and insertion curves (Petsiuk et al. 2018) of an attribution for target[clip] on b clips, b may
        exceed max_batch: the cells of grid = (gt, gh, gw) (default (T, 1, 1): the frames) are frozen per pixel
        (deletion) or released from the fully frozen clip (insertion) in the order the attribution ranks them, `step`
        cells per forward.  Returns a dict of device tensors: curve_ranks int16 [b,P], del_scores, ins_scores [b,J+1],
        del_auc, ins_auc, del_auc_norm, ins_auc_norm [b], score_x [b] (the plan's ordinary forward).  A faithful
        attribution under 'morf' has a low deletion and a high insertion AUC."""
        gt, gh, gw, step, _, order, _, _ = self._curve_args(grid, sigma, step, 3, order)
        x = self._clip(x, any_batch=True)
        b = x.shape[0]
        tgt = self._targets(target, b)
        score_x = self._score_x(x, tgt)
        ranks = self.curve_ranks(attr, (gt, gh, gw), sigma, order)
        if ranks.shape[0] != b:
            raise L.IvfError(f"need an attribution for each of the {b} clips, got {ranks.shape[0]}")
        scores = self.curve_scores(x, tgt, ranks, (gt, gh, gw), sigma, step, 3)
        auc, norm = self.curve_reduce(scores, (gt, gh, gw), step, 3)
        return dict(curve_ranks=ranks, del_scores=scores[:, 0], ins_scores=scores[:, 1], del_auc=auc[:, 0],
                    ins_auc=auc[:, 1], del_auc_norm=norm[:, 0], ins_auc_norm=norm[:, 1], score_x=score_x)

    def argmax(self, probs):
        b = probs.shape[0]
        t = torch.empty(b, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().ivf_argmax(L.ptr(L.f32c(probs)), b, probs.shape[1], L.ptr(t), L.stream()))
        return t


class I3DEngine(_Engine):
    """Plan + arenas for `models.I3D_doubled{,_kth}.Model` on `max_batch` clips of
    geometry [C,T,H,W] (reference Model.forward, I3D_doubled.py:351-380)."""
    _prefix = "i3d"

    def __init__(self, num_classes, clip_shape, max_batch=1, stride_mod_layers="", last_stride=1,
                 head_hw=(7, 7), head_time_base=2, softmax=True, device=None, math=None):
        super().__init__(num_classes, clip_shape, max_batch, device)
        sml = arch.parse_stride_mod(stride_mod_layers)
        cfg = L.I3DConfig()
        cfg.stem_stride_t = arch.temporal_stride('Conv3d_1a_7x7', sml, last_stride)
        cfg.pool4a_stride_t = arch.temporal_stride('MaxPool3d_4a_3x3', sml, last_stride)
        cfg.pool5a_stride_t = arch.temporal_stride('MaxPool3d_5a_2x2', sml, last_stride)
        cfg.head_kt = arch.head_time_kernel(sml, last_stride, head_time_base)
        cfg.head_kh, cfg.head_kw = head_hw
        cfg.softmax = 1 if softmax else 0
        self.math = math if math is not None else DEFAULT_MATH
        cfg.math = L.MATH_MODES[self.math]
        self._create(cfg)
        self._tuned = False
        self.unit_names = []
        for i in range(L.lib().ivf_i3d_num_convs(self._h)):
            name = ctypes.create_string_buffer(64)
            L.check(L.lib().ivf_i3d_conv_info(self._h, i, name, None, None, None, None, None, None))
            self.unit_names.append(name.value.decode())

    # -------------------------------------------------------------- weights
    def load_state_dict(self, sd, bn_eps=1e-3, autotune=None):
        """sd: reference key scheme, optional 'module.' prefix."""
        def get(key):
            return self._param(sd, key)
        keep = []
        with torch.cuda.device(self.device):
            for i, name in enumerate(self.unit_names):
                w = get(f"{name}.conv3d.weight")
                if name == "logits":
                    bias = get("logits.conv3d.bias")
                    keep += [w, bias]
                    L.check(L.lib().ivf_i3d_load_conv(self._h, i, L.ptr(w), None, None, None, None,
                                                      L.ptr(bias), bn_eps, L.stream()))
                else:
                    g, b = get(f"{name}.bn.weight"), get(f"{name}.bn.bias")
                    m, v = get(f"{name}.bn.running_mean"), get(f"{name}.bn.running_var")
                    keep += [w, g, b, m, v]
                    L.check(L.lib().ivf_i3d_load_conv(self._h, i, L.ptr(w), L.ptr(g), L.ptr(b), L.ptr(m),
                                                      L.ptr(v), None, bn_eps, L.stream()))
            torch.cuda.current_stream().synchronize()   # sources may be freed after this
        if (AUTOTUNE if autotune is None else autotune) and not self._tuned:
            self.autotune()

    # -------------------------------------------------------------- kernel selection
    def autotune(self, reps=3, sample=None):
        """Time every kernel variant of every convolution at the plan's batch size and keep the
        fastest per layer and direction.  Results: see get_tuning / set_tuning.

        The candidates are timed on the plan's own activation / gradient buffers, so these are filled first by one
        forward + backward of `sample` (a [max_batch,C,T,H,W] clip batch; default: seeded noise in [-1, 1]): on an
        untouched (all-zero) workspace the matrix pipe toggles nothing, the chip holds a higher clock and the
        MFMA-dense tiles rank 16-19 % better than they run on data (MI355X_MICROARCH.md, DVFS give-back)."""
        with torch.cuda.device(self.device):
            if sample is None:
                g = torch.Generator(device="cpu").manual_seed(0)
                one = torch.rand((1,) + tuple(self.clip_shape), generator=g) * 2.0 - 1.0
                sample = one.to(self.device).expand(self.max_batch, *self.clip_shape).contiguous()
            probs = self.forward(sample)
            self.backward(sample.shape[0], target=self.argmax(probs), want_dx=False)
            del sample, probs
            L.check(L.lib().ivf_i3d_autotune(self._h, self.max_batch, int(reps), L.stream()))
            torch.cuda.current_stream().synchronize()
        self._tuned = True

    def set_overlap(self, on):
        """Run the HBM-bound branch of every Inception module on a side stream beside the 3x3x3 convs
        (ivf_i3d_set_overlap; off by default, bit-identical results)."""
        L.check(L.lib().ivf_i3d_set_overlap(self._h, int(bool(on))))

    def get_tuning(self):
        n = 2 * L.lib().ivf_i3d_num_conv_ops(self._h)
        arr = (c_int * n)()
        L.check(L.lib().ivf_i3d_get_tuning(self._h, arr))
        return list(arr)

    def set_tuning(self, variants):
        n = 2 * L.lib().ivf_i3d_num_conv_ops(self._h)
        if len(variants) != n:
            raise L.IvfError(f"tuning vector must have {n} entries")
        arr = (c_int * n)(*[int(v) for v in variants])
        L.check(L.lib().ivf_i3d_set_tuning(self._h, arr))
        self._tuned = True

    # -------------------------------------------------------------- entry points of this backbone alone
    def endpoint(self, name, b):
        """Activation of the last forward as an NCTHW torch tensor (copy)."""
        p = c_void_p()
        T, H, W, C, ld = c_int(), c_int(), c_int(), c_int(), c_int()
        L.check(L.lib().ivf_i3d_endpoint(self._h, name.encode(), byref(p), byref(T), byref(H), byref(W),
                                         byref(C), byref(ld)))
        off = p.value - self._ws.data_ptr()
        n = b * T.value * H.value * W.value * ld.value
        esz = L.lib().ivf_i3d_act_elem_bytes(self._h)           # 2: bf16 storage (math="bf16act")
        if name.split(":")[0] == "input":
            esz = 4                                             # the clip and its gradient stay fp32 in every mode
        flat = self._ws[off:off + esz * n].view(torch.float32 if esz == 4 else torch.bfloat16).float()
        return flat.view(b, T.value, H.value, W.value, ld.value)[..., :C.value].permute(0, 4, 1, 2, 3).contiguous()

    def gradcam(self, x, target=None, per_frame=True, out_hw=None, layer="Mixed_5c"):
        """GradCamVideo for b clips: (cam [b,T,H,W], probs [b,K]).  `layer`: the target endpoint
        (Conv3d_1a_7x7 ... Mixed_5c; the reference drivers use Mixed_5c, smth:258)."""
        x = self._clip(x)
        b = x.shape[0]
        C, T, H, W = self.clip_shape
        oh, ow = out_hw if out_hw is not None else (H, W)
        if target is None:
            target = self.argmax(self.forward(x))
        tgt = self._targets(target, b)
        p = c_void_p()
        Tf = c_int()
        if "." in layer or layer == "input":
            raise L.IvfError(f"'{layer}' is not an endpoint of the model")
        L.check(L.lib().ivf_i3d_endpoint(self._h, layer.encode(), byref(p), byref(Tf), None, None, None, None))
        frames = Tf.value * (T // Tf.value)
        cam = torch.empty(b, frames, oh, ow, device=self.device)
        probs = torch.empty(b, self.K, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().ivf_i3d_gradcam_layer(self._h, L.ptr(x), b, L.ptr(tgt), layer.encode(),
                                                  1 if per_frame else 0, oh, ow, L.ptr(cam), L.ptr(probs), L.stream()))
        return cam, probs

    def _cam_endpoint(self, layer):
        """(T', H', W', C) of an endpoint that can be a CAM target."""
        if "." in layer or ":" in layer or layer == "input":
            raise L.IvfError(f"'{layer}' is not an endpoint of the model")
        p = c_void_p()
        v = [c_int() for _ in range(4)]
        L.check(L.lib().ivf_i3d_endpoint(self._h, layer.encode(), byref(p), *[byref(a) for a in v], None))
        return tuple(a.value for a in v)

    def cam(self, x, target=None, kinds=("gradcam",), per_frame=True, out_hw=None, layer="Mixed_5c"):
        """The Grad-CAM family from ONE forward and ONE backward: ({kind: cam [b,T,H,W]}, probs [b,K]) for
        the kinds of 'gradcam', 'gradcam++', 'xgradcam', 'hirescam', 'layercam' asked for; arguments as `gradcam`."""
        x = self._clip(x)
        b = x.shape[0]
        C, T, H, W = self.clip_shape
        oh, ow = out_hw if out_hw is not None else (H, W)
        kinds, ids = L.cam_kind_ids(kinds)
        Tf = self._cam_endpoint(layer)[0]
        if target is None:
            target = self.argmax(self.forward(x))
        tgt = self._targets(target, b)
        cam = torch.empty(len(kinds), b, Tf * (T // Tf), oh, ow, device=self.device)
        probs = torch.empty(b, self.K, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().ivf_i3d_cam_layer(self._h, L.ptr(x), b, L.ptr(tgt), layer.encode(), len(kinds), ids,
                                              1 if per_frame else 0, oh, ow, L.ptr(cam), L.ptr(probs), L.stream()))
        return {k: cam[i] for i, k in enumerate(kinds)}, probs

    def cam_raw(self, x, target=None, kinds=("gradcam",), layer="Mixed_5c"):
        """The pieces of `cam` before the resize: {kind: dict(cam [b,T',H',W'], weights [b,C])} plus, under 'feat' and
        'grad', fp32 copies [b,T',H',W',C] of the activations and gradients the reduction read, and 'probs' [b,K]."""
        x = self._clip(x)
        b = x.shape[0]
        kinds, ids = L.cam_kind_ids(kinds)
        Tf, Hf, Wf, Cf = self._cam_endpoint(layer)
        if target is None:
            target = self.argmax(self.forward(x))
        tgt = self._targets(target, b)
        dev = self.device
        cam = torch.empty(len(kinds), b, Tf, Hf, Wf, device=dev)
        wts = torch.empty(len(kinds), b, Cf, device=dev)
        out = dict(feat=torch.empty(b, Tf, Hf, Wf, Cf, device=dev), grad=torch.empty(b, Tf, Hf, Wf, Cf, device=dev),
                   probs=torch.empty(b, self.K, device=dev))
        with torch.cuda.device(dev):
            L.check(L.lib().ivf_i3d_cam_raw(self._h, L.ptr(x), b, L.ptr(tgt), layer.encode(), len(kinds), ids,
                                            L.ptr(cam), L.ptr(wts), L.ptr(out["feat"]), L.ptr(out["grad"]),
                                            L.ptr(out["probs"]), L.stream()))
        for i, k in enumerate(kinds):
            out[k] = dict(cam=cam[i], weights=wts[i])
        return out

    def _scorecam_feat(self, layer):
        layer = "Mixed_5c" if layer is None else layer
        Tf, Hf, Wf, Cf = self._cam_endpoint(layer)
        return (f"'{layer}'", (Cf, Tf, Hf, Wf),
                lambda x: self.cam_raw(x, None, layer=layer)["feat"].permute(0, 4, 1, 2, 3))


class CLSTMEngine(_Engine):
    """Plan + arenas for `models.CLSTM_4.Model` (reference CLSTM_4.py:69-85 over
    convolution_lstm.py:96-132) on `max_batch` clips [C,T,H,W]."""
    _prefix = "clstm"

    def __init__(self, num_classes, clip_shape, max_batch=1, hidden=4, layers=2, kernel=5, stride=2,
                 softmax=False, batch_norm=True, out_step=None, out_steps=None, device=None, effective_steps=None):
        """effective_steps: the effective steps inside the clip (convolution_lstm.py:129-130), whose top-layer
        outputs are the map stack of Grad-CAM target 'clstm'; default: the steps that feed endFC."""
        super().__init__(num_classes, clip_shape, max_batch, device)
        T = clip_shape[1]
        cfg = L.CLSTMConfig()
        cfg.hidden, cfg.layers, cfg.kernel, cfg.stride = int(hidden), int(layers), int(kernel), int(stride)
        cfg.softmax = 1 if softmax else 0
        cfg.batch_norm = 1 if batch_norm else 0
        cfg.out_step = T - 1 if out_step is None else int(out_step)
        if out_steps is not None:           # use_entire_seq: every effective step reached feeds endFC
            if not 1 <= len(out_steps) <= 16:
                raise L.IvfError("between 1 and 16 output steps")
            cfg.n_out_steps = len(out_steps)
            for i, sv in enumerate(out_steps):
                cfg.out_steps[i] = int(sv)
            cfg.out_step = int(out_steps[-1])
        self.layers = int(layers)
        self._create(cfg)
        if effective_steps is None:
            effective_steps = list(out_steps) if out_steps is not None else [cfg.out_step]
        self.effective_steps = tuple(int(v) for v in effective_steps)
        L.check(L.lib().ivf_clstm_set_cam_steps(self._h, (c_int * len(self.effective_steps))(*self.effective_steps),
                                                len(self.effective_steps)))

    def load_state_dict(self, sd, bn_eps=1e-5):
        def get(key):
            return self._param(sd, key)
        with torch.cuda.device(self.device):
            for i in range(self.layers):
                ts = ([get(f"clstm.cell{i}.Wx{g}.weight") for g in "ifco"]
                      + [get(f"clstm.cell{i}.Wx{g}.bias") for g in "ifco"]
                      + [get(f"clstm.cell{i}.Wh{g}.weight") for g in "ifco"])
                L.check(L.lib().ivf_clstm_load_cell(self._h, i, *[L.ptr(t) for t in ts], L.stream()))
                torch.cuda.current_stream().synchronize()
            bn = [get(f"clstm.bn.{k}") for k in ("weight", "bias", "running_mean", "running_var")] \
                if self.cfg.batch_norm else [None] * 4
            fw, fb = get("endFC.weight"), get("endFC.bias")
            L.check(L.lib().ivf_clstm_load_head(self._h, *[L.ptr(t) for t in bn], L.ptr(fw), L.ptr(fb), bn_eps,
                                                L.stream()))
            torch.cuda.current_stream().synchronize()

    def backward(self, b, target=None, dout=None, want_dx=True):
        return super().backward(b, target, dout, True)      # this plan always writes dx

    # ------------------------------------------------------------ Grad-CAM
    def _cam_layer(self, layer):
        """layer None -> -1 (the reference's stack of effective steps), int i -> per-frame maps of layer i."""
        if layer is None:
            return -1, len(self.effective_steps)
        if isinstance(layer, bool) or not isinstance(layer, (int, np.integer)) or not 0 <= int(layer) < self.layers:
            raise L.IvfError(f"Grad-CAM layer must be None or an int in [0,{self.layers}), got {layer!r}")
        return int(layer), self.clip_shape[1]

    def layer_dims(self, layer):
        """(hid, Hp, Wp) of a layer's pooled output."""
        v = [c_int() for _ in range(3)]
        L.check(L.lib().ivf_clstm_layer_buffers(self._h, int(layer), None, None, *[byref(a) for a in v]))
        return tuple(a.value for a in v)

    def layer_state(self, layer, b):
        """Copies of what the last forward / backward left for a layer: pooled outputs and their gradient,
        both [b,T,hid,Hp,Wp]."""
        X, dX = c_void_p(), c_void_p()
        L.check(L.lib().ivf_clstm_layer_buffers(self._h, int(layer), byref(X), byref(dX), None, None, None))
        hid, Hp, Wp = self.layer_dims(layer)
        T = self.clip_shape[1]
        n = b * T * hid * Hp * Wp
        out = []
        for p in (X, dX):
            off = p.value - self._ws.data_ptr()
            out.append(self._ws[off:off + 4 * n].view(torch.float32).view(b, T, hid, Hp, Wp).clone())
        return tuple(out)

    def gradcam(self, x, target=None, per_frame=True, out_hw=None, layer=None):
        """GradCamVideo for b clips: (cam [b,frames,H,W], probs [b,K]), the I3D engine's convention.

        layer=None is the reference's CLSTM branch (grad-cam.py:33-49, grad_cam_videos.py:88-142): the top layer's
        pooled outputs at the effective steps with the gradient endFC sends into them, n_eff maps each repeated
        T // n_eff times.  layer=i is an EXTENSION (no counterpart in the reference, pinned by autograd on the
        reference's model): layer i's pooled output at every step with the gradient of the class score through
        the layers above and their recurrences; T per-frame maps that line up with the temporal mask."""
        x = self._clip(x)
        b = x.shape[0]
        C, T, H, W = self.clip_shape
        oh, ow = out_hw if out_hw is not None else (H, W)
        li, n = self._cam_layer(layer)
        tgt = self._targets(target, b) if target is not None else None     # None: argmax on the device
        cam = torch.empty(b, n * (T // n), oh, ow, device=self.device)
        probs = torch.empty(b, self.K, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().ivf_clstm_gradcam(self._h, L.ptr(x), b, L.ptr(tgt), li, 1 if per_frame else 0, int(oh),
                                              int(ow), L.ptr(cam), L.ptr(probs), L.stream()))
        return cam, probs

    def gradcam_raw(self, x, target=None, layer=None):
        """The pieces of `gradcam` before the resize: dict of cam [b,n,Hp,Wp], weights [b,hid], feat and grad
        [b,n,hid,Hp,Wp] (the features and gradients the reduction read) and probs [b,K]."""
        x = self._clip(x)
        b = x.shape[0]
        li, n = self._cam_layer(layer)
        hid, Hp, Wp = self.layer_dims(self.layers - 1 if li < 0 else li)
        tgt = self._targets(target, b) if target is not None else None
        dev = self.device
        out = dict(cam=torch.empty(b, n, Hp, Wp, device=dev), weights=torch.empty(b, hid, device=dev),
                   feat=torch.empty(b, n, hid, Hp, Wp, device=dev), grad=torch.empty(b, n, hid, Hp, Wp, device=dev),
                   probs=torch.empty(b, self.K, device=dev))
        with torch.cuda.device(dev):
            L.check(L.lib().ivf_clstm_gradcam_raw(self._h, L.ptr(x), b, L.ptr(tgt), li, L.ptr(out["cam"]),
                                                  L.ptr(out["weights"]), L.ptr(out["feat"]), L.ptr(out["grad"]),
                                                  L.ptr(out["probs"]), L.stream()))
        return out

    def cam(self, x, target=None, kinds=("gradcam",), per_frame=True, out_hw=None, layer=None):
        """The Grad-CAM family from ONE forward and ONE backward: ({kind: cam [b,frames,H,W]}, probs);
        arguments as `gradcam`."""
        x = self._clip(x)
        b = x.shape[0]
        C, T, H, W = self.clip_shape
        oh, ow = out_hw if out_hw is not None else (H, W)
        kinds, ids = L.cam_kind_ids(kinds)
        li, n = self._cam_layer(layer)
        tgt = self._targets(target, b) if target is not None else None
        cam = torch.empty(len(kinds), b, n * (T // n), oh, ow, device=self.device)
        probs = torch.empty(b, self.K, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().ivf_clstm_cam(self._h, L.ptr(x), b, L.ptr(tgt), li, len(kinds), ids, 1 if per_frame else 0,
                                          int(oh), int(ow), L.ptr(cam), L.ptr(probs), L.stream()))
        return {k: cam[i] for i, k in enumerate(kinds)}, probs

    def cam_raw(self, x, target=None, kinds=("gradcam",), layer=None):
        """The pieces of `cam` before the resize: {kind: dict(cam [b,n,Hp,Wp], weights [b,hid])} plus 'feat' and 'grad'
        [b,n,hid,Hp,Wp] (what the reduction read) and 'probs' [b,K]."""
        x = self._clip(x)
        b = x.shape[0]
        kinds, ids = L.cam_kind_ids(kinds)
        li, n = self._cam_layer(layer)
        hid, Hp, Wp = self.layer_dims(self.layers - 1 if li < 0 else li)
        tgt = self._targets(target, b) if target is not None else None
        dev = self.device
        cam = torch.empty(len(kinds), b, n, Hp, Wp, device=dev)
        wts = torch.empty(len(kinds), b, hid, device=dev)
        out = dict(feat=torch.empty(b, n, hid, Hp, Wp, device=dev), grad=torch.empty(b, n, hid, Hp, Wp, device=dev),
                   probs=torch.empty(b, self.K, device=dev))
        with torch.cuda.device(dev):
            L.check(L.lib().ivf_clstm_cam_raw(self._h, L.ptr(x), b, L.ptr(tgt), li, len(kinds), ids, L.ptr(cam),
                                              L.ptr(wts), L.ptr(out["feat"]), L.ptr(out["grad"]), L.ptr(out["probs"]),
                                              L.stream()))
        for i, k in enumerate(kinds):
            out[k] = dict(cam=cam[i], weights=wts[i])
        return out

    def _scorecam_feat(self, layer):
        li, n = self._cam_layer(layer)
        hid, Hp, Wp = self.layer_dims(self.layers - 1 if li < 0 else li)
        return ("'clstm'" if li < 0 else f"'cell{li}'", (hid, n, Hp, Wp),
                lambda x: self.cam_raw(x, None, layer=layer)["feat"].permute(0, 2, 1, 3, 4))


class TFCLSTMEngine(_Engine):
    """SURVEY 8f N4, a DOCUMENTED EXTENSION (parity unpinned): the TF half's Keras ConvLSTM2D classifier
    (video_features_tf/models/clstm.py:87-126) and its temporal-mask search / per-frame Grad-CAM
    (mask/find_mask_kth.py:300-452, mask/gradcam.py:28-111) on libivf_hip's generic direct-convolution kernels
    (csrc/tf_clstm.hip).  Clips are NCTHW like everywhere else; `from_tf_layout` converts [B,T,H,W,C].
    The plan perturbs by freezing only and has no one-blob entry (the inherited `blob_scores` finds no symbol); `ig`,
    `ig_path_scores`, the `rise*`, `shap*` and `curve*` entries, `faithfulness`, `smoothgrad`, `sg_noise`, `kernelshap`,
    `lime` and their row entries refuse with IvfError."""
    _prefix = "tfclstm"
    _has_mode = False
    _has_st = False
    _has_ig = False

    def __init__(self, num_classes, clip_shape, units=(32, 32), kernel=(3, 5), stride=2, padding="valid",
                 recurrent_activation="hard_sigmoid", only_last_element_for_fc=True, max_batch=1, device=None):
        super().__init__(num_classes, clip_shape, max_batch, device)
        cfg = L.TFCLSTMConfig()
        cfg.layers = len(units)
        for i, u in enumerate(units):
            cfg.units[i] = int(u)
        cfg.kh, cfg.kw = int(kernel[0]), int(kernel[1])
        cfg.stride = int(stride)
        if padding not in ("valid", "same"):
            raise L.IvfError("padding must be 'valid' or 'same'")
        cfg.padding = 1 if padding == "same" else 0
        if recurrent_activation not in ("hard_sigmoid", "sigmoid"):
            raise L.IvfError("recurrent_activation must be 'hard_sigmoid' or 'sigmoid'")
        cfg.recurrent_hard_sigmoid = 1 if recurrent_activation == "hard_sigmoid" else 0
        cfg.only_last = 1 if only_last_element_for_fc else 0
        self.units = tuple(int(u) for u in units)
        self._create(cfg)

    @staticmethod
    def from_tf_layout(x_bthwc):
        """[B,T,H,W,C] (the TF graph's sequence layout) -> NCTHW."""
        return x_bthwc.permute(0, 4, 1, 2, 3).contiguous()

    @property
    def fc_inputs(self):
        return L.lib().ivf_tfclstm_fc_inputs(self._h)

    def layer_dims(self, i):
        v = [c_int() for _ in range(5)]
        L.check(L.lib().ivf_tfclstm_layer_dims(self._h, i, *[byref(a) for a in v]))
        return tuple(a.value for a in v)

    def layer_state(self, layer, b):
        """Copies of what the last forward / backward left for a block (test support): its output sequence H
        [b,T,F,Ho,Wo], its pooled output X and the gradient dX that arrived at X, both [b,T,F,Hp,Wp]."""
        H, X, dX = c_void_p(), c_void_p(), c_void_p()
        L.check(L.lib().ivf_tfclstm_layer_buffers(self._h, int(layer), byref(H), byref(X), byref(dX)))
        Ho, Wo, Hp, Wp, Fu = self.layer_dims(layer)
        T = self.clip_shape[1]
        out = []
        for p, (h, w) in ((H, (Ho, Wo)), (X, (Hp, Wp)), (dX, (Hp, Wp))):
            off = p.value - self._ws.data_ptr()
            n = b * T * Fu * h * w
            out.append(self._ws[off:off + 4 * n].view(torch.float32).view(b, T, Fu, h, w).clone())
        return tuple(out)

    def load_weights(self, layers, dense_w, dense_b):
        """layers: [(kernel [kh,kw,Cin,4F], recurrent_kernel [kh,kw,F,4F], bias [4F])] in Keras layouts;
        dense_w [inputs, classes], dense_b [classes]."""
        dev = self.device
        with torch.cuda.device(dev):
            for i, (k, rk, b) in enumerate(layers):
                k, rk, b = (L.f32c(torch.as_tensor(t).to(dev)) for t in (k, rk, b))
                L.check(L.lib().ivf_tfclstm_load_layer(self._h, i, L.ptr(k), L.ptr(rk), L.ptr(b), L.stream()))
                torch.cuda.current_stream().synchronize()
            dw, db = L.f32c(torch.as_tensor(dense_w).to(dev)), L.f32c(torch.as_tensor(dense_b).to(dev))
            if tuple(dw.shape) != (self.fc_inputs, self.K):
                raise L.IvfError(f"dense kernel must be [{self.fc_inputs},{self.K}], got {tuple(dw.shape)}")
            L.check(L.lib().ivf_tfclstm_load_head(self._h, L.ptr(dw), L.ptr(db), L.stream()))
            torch.cuda.current_stream().synchronize()

    def backward(self, b, target):
        C, T, H, W = self.clip_shape
        tgt = self._targets(target, b)
        score = torch.empty(b, device=self.device)
        dx = torch.empty(b, C, T, H, W, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().ivf_tfclstm_backward(self._h, b, L.ptr(tgt), L.ptr(score), L.ptr(dx), L.stream()))
        return score, dx

    def perturbed_forward(self, x, mask):
        return super().perturbed_forward(x, mask)

    def search(self, x, target, raw_mask, lam1, lam2, N, lr=0.2, betas=(0.9, 0.999), eps=1e-8, state=None):
        return super().search(x, target, raw_mask, lam1, lam2, N, lr, betas, eps, state)

    def gradcam(self, x, target, mask=None, normalization_mode="frame", out_hw=None):
        """mask/gradcam.py: per-frame maps [b,T,H,W]; normalization_mode 'frame' | 'sequence' (FLAGS.normalization_mode)."""
        x = self._clip(x)
        b = x.shape[0]
        C, T, H, W = self.clip_shape
        oh, ow = out_hw if out_hw is not None else (H, W)
        if normalization_mode not in ("frame", "sequence"):
            raise L.IvfError("Error. Need to provide normalization mode.")           # gradcam.py:97
        tgt = self._targets(target, b)
        m = L.f32c(mask.to(self.device)) if mask is not None else None
        cam = torch.empty(b, T, oh, ow, device=self.device)
        probs = torch.empty(b, self.K, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().ivf_tfclstm_gradcam(self._h, L.ptr(x), b, L.ptr(m), L.ptr(tgt), 1 if normalization_mode == "frame" else 0,
                                                oh, ow, L.ptr(cam), L.ptr(probs), L.stream()))
        return cam, probs
