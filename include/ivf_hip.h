/* libivf_hip.so -- C-ABI of the MI355X (gfx950) video-saliency hot path.
 *
 * The reference (interpreting-video-features) has no FFI/plugin boundary: its hot
 * path is plain PyTorch called from Python.  This header is therefore the
 * build-defined boundary beneath the reference's Python call surface (SURVEY.md
 * section 8b); each entry point names the reference code it replaces.  File:line
 * citations are relative to /root/reference/video_features_pytorch/ ("smth" =
 * FindMasksComparison_I3D_smth.py).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to fp32 unless its name ends in _host or
 *    its type says otherwise; the caller owns all memory, the library never
 *    allocates or frees device memory; scratch is passed in, sized by the
 *    matching *_workspace_bytes() query;
 *  - `stream` is a hipStream_t (0 = the null stream); every call only enqueues
 *    work and never synchronises, so a call sequence can be captured in a hipGraph;
 *  - return value 0 = ok, negative = error (IVF_ERR_*), message via
 *    ivf_last_error() (thread-local);
 *  - activations inside the library are channels-last [B, T, H, W, ld] fp32 with a
 *    channel window (coff, C) inside the row of ld floats; reference tensors are
 *    NCTHW [B, C, T, H, W] and are converted at the edges (freeze/reverse kernels
 *    write channels-last directly).
 */
#ifndef IVF_HIP_H
#define IVF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IVF_OK 0
#define IVF_ERR_BAD_ARG (-1)
#define IVF_ERR_HIP (-2)
#define IVF_ERR_UNSUPPORTED (-3)

typedef void* ivf_stream_t; /* hipStream_t */

const char* ivf_last_error(void);
int ivf_version(void);

/* ------------------------------------------------------------------ mask.py */

/* mask.perturb_sequence(..., 'freeze') forward, mask.py:11-22.
 * x [B,C,T,HW] NCTHW; mask [T] (mask_per_clip=0) or [B,T] (=1), already in [0,1];
 * p: out_cpad==0 -> NCTHW, else channels-last [B,T,HW,out_cpad] (pad channels zero). */
int ivf_freeze_fwd(const float* x, const float* mask, float* p, int B, int C, int T, int HW,
                   int mask_per_clip, int out_cpad, ivf_stream_t stream);

/* Backward of the same (autograd of mask.py:11-22 under smth:213).
 * g: upstream gradient, NCTHW (g_cpad==0) or channels-last with row g_cpad.
 * dmask [B,T] per-clip gradient (sum over B yourself for a shared mask; entry 0 is 0);
 * dx NCTHW or NULL.  Deterministic two-stage reduction (no float atomics). */
size_t ivf_freeze_bwd_workspace_bytes(int B, int T);
int ivf_freeze_bwd(const float* x, const float* mask, const float* g, float* dmask, float* dx, int B,
                   int C, int T, int HW, int mask_per_clip, int g_cpad, void* workspace,
                   ivf_stream_t stream);

/* find_submasks_from_mask, mask.py:60-85, plus the pairing rule of the 'reverse'
 * perturbation, mask.py:40-56.  run[t] = index of the run containing frame t or -1;
 * partner[t] = frame swapped with t (t itself if copied); weight[t] = mask value of
 * the pair's first-half member (used for BOTH members, mask.py:50-56). */
int ivf_submask_pairs(const float* mask, int T, float thresh, int* run, int* partner, float* weight,
                      ivf_stream_t stream);

/* mask.perturb_sequence(..., 'reverse') given the pairing above. */
int ivf_reverse_fwd(const float* x, const int* partner, const float* weight, float* p, int B, int C,
                    int T, int HW, int out_cpad, ivf_stream_t stream);

/* The same for b clips with per-clip masks [B,T] (partner/weight rows [B,T]); forward writes
 * NCTHW (out_cpad 0) or 16-byte channels-last pixels (out_cpad 4). */
int ivf_submask_pairs_batched(const float* mask, int B, int T, float thresh, int* partner, float* weight,
                              ivf_stream_t stream);
int ivf_reverse_fwd_batched(const float* x, const int* partner, const float* weight, float* p, int B, int C,
                            int T, int HW, int out_cpad, ivf_stream_t stream);
/* Autograd of mask.py:49-56 w.r.t. the mask (the reference optimises through 'reverse' when
 * temporalMaskType == 'reverse', smth:121,202): for a pair (a, b'), a in the first half of its run,
 * dmask[a] = sum (X[b'] - X[a]) * (G[a] - G[b']); all other entries 0.  g NCTHW (g_cpad 0) or
 * channels-last; workspace: ivf_freeze_bwd_workspace_bytes(B, T). */
int ivf_reverse_bwd(const float* x, const int* partner, const float* g, float* dmask, int B, int C, int T,
                    int HW, int g_cpad, void* workspace, ivf_stream_t stream);

/* mask.calc_tv_norm(mask, p, q), mask.py:88-100: val[b] and (optional) grad[b,:]. */
int ivf_tv_norm(const float* mask, int B, int T, float p, float q, float* val, float* grad,
                ivf_stream_t stream);

/* Regulariser of the search loop, smth:198-200: sig = sigmoid(raw);
 * terms[b] = {lam1*sum|sig|, lam2*TV33(sig)}; dreg_dsig = d(l1+tv)/dsig. */
int ivf_mask_reg(const float* raw_mask, int B, int T, float lam1, float lam2, float* sig, float* terms,
                 float* dreg_dsig, ivf_stream_t stream);

/* torch.optim.Adam step on one tensor (smth:191,214); step counts from 1. */
int ivf_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int n, int step,
                  float lr, float beta1, float beta2, float eps, ivf_stream_t stream);

/* Loop tail, smth:207-214: chain through the sigmoid, Adam step on raw_mask [B,T],
 * traj_row[b] = (loss, l1, tv, score). */
int ivf_search_step(float* raw_mask, const float* sig, const float* dscore_dsig, const float* dreg_dsig,
                    const float* terms, const float* score, float* exp_avg, float* exp_avg_sq,
                    float* traj_row, int B, int T, int step, float lr, float beta1, float beta2,
                    float eps, ivf_stream_t stream);

int ivf_sigmoid(const float* x, float* y, int n, ivf_stream_t stream);

/* Integer frame-importance ranking of finished masks (the drivers rank frames by mask value,
 * FindMasksComparison_I3D_smth.py:216-230): order[b][r] = frame with the r-th largest value of mask[b][:], ties by
 * frame index, NaN last -- torch.argsort(-mask, stable=True).  mask [B,T] fp32, order [B,T] int32. */
int ivf_rank_frames(const float* mask, int B, int T, int* order, ivf_stream_t stream);

/* init_mask(mode='central') selection for B clips (mask.py:134-154): orig[b] / full[b] = target score of the clip /
 * of its fully frozen version, central[b][i] = score under candidate i+1 (ones with i+1 zeros at each end), n
 * candidates.  ratio[b][i] = (orig - central) / (orig - full) (optional output); chosen_i[b] (optional, 1-based) = first
 * candidate whose ratio < threshold, else n (NaN compares false, as in the reference); raw_mask[b][t] = -5 on the
 * chosen candidate's zeros, +5 on its ones. */
int ivf_init_central_select(const float* orig, const float* full, const float* central, int B, int n, int T,
                            float threshold, float* raw_mask, int* chosen_i, float* ratio, ivf_stream_t stream);

/* Exhaustive one-blob temporal mask search, maskType 'combi' (find_masks docstring, smth:137-141: "iterate through
 * the different combinations of a coherent 'one blob' mask.  Does not use grad desc").  Candidates are the binary
 * masks m_{a,L} = 1 on [a, a+L), 1 <= L <= max_len, 0 <= a <= T-L, in canonical order L ascending then a ascending:
 * k(a,L) = sum_{l<L} (T-l+1) + a.  At a binary mask both perturbations are frame gathers: freeze puts frame
 * max(a-1,0) on the blob (mask.py:11-22), reverse puts frame 2a+L-1-u on frame u (mask.py:24-56).
 * ivf_blob_count: host, n = sum_{L=1}^{max_len} (T-L+1), or -1 (message set) unless 1 <= max_len <= T <= 64. */
int ivf_blob_count(int T, int max_len);
/* Write candidates [first, first+count) of the flattened (clip, candidate) list of b clips x [b,C,T,HW] (row j =
 * clip (first+j)/n, candidate (first+j)%n) into p: out_cpad 4 = the I3D plan's input layout [count,T,HW,4]
 * (16-byte pixels, C <= 4), out_cpad 0 = NCTHW [count,C,T,HW].  mode 0 freeze, 1 reverse. */
int ivf_blob_stage(const float* x, int b, int C, int T, int HW, int max_len, int mode, long long first, int count,
                   float* p, int out_cpad, ivf_stream_t stream);
/* Selection over a score grid scores [b,n] (n = ivf_blob_count(T, max_len)), one clip per thread:
 * J_k = lam1*sum(m_k) + lam2*TV33(m_k) + s_k with the search loop's fp32 regulariser (ivf_mask_reg), obj [b,n]
 * (optional); best [b,2] = (a,L) of argmin J, ties to the smaller L then the smaller a, NaN skipped, best_obj [b]
 * (optional); minimal [b,2] (optional) = init_mask('central')'s criterion (mask.py:121-154) over one-blob masks:
 * r = (orig - s) / (orig - full), the smallest L with some r >= threshold, the largest r within it, then the smaller
 * a; (-1,-1) if none qualifies. */
int ivf_blob_select(const float* scores, const float* orig, const float* full, int b, int T, int max_len, float lam1,
                    float lam2, float threshold, int* best, float* best_obj, float* obj, int* minimal,
                    ivf_stream_t stream);

/* ------------------------------------------------------------------ spatio-temporal masks (maskType 'spacetime')
 * An EXTENSION with no counterpart in the reference, pinned by torch autograd on the reference's models:
 * the freeze perturbation with a mask value per pixel and frame, parametrised per frame on a coarse gh x gw grid
 * (gh, gw <= 32).  S = sigmoid(R), R [B,T,gh,gw];  M[b,t] = A_H S[b,t] A_W^T, M [B,T,H,W];
 * P[0] = X[0], P[u] = (1 - M[u]) X[u] + M[u] P[u-1] per pixel.  No float atomics: every sum has a fixed order and a
 * clip's results do not depend on the batch it ran in.
 *
 * ivf_stmask_axis_weights: HOST.  A [n_out,n_in] = G U in fp64, rounded once to fp32: U bilinear upsampling with
 * half-pixel centres and clamped edges (F.interpolate(mode='bilinear', align_corners=False)), G a Gaussian of radius
 * ceil(3 sigma) in output pixels, taps normalised to sum 1, replicated border; sigma == 0 gives A = U.  Entries >= 0,
 * rows sum to 1. */
int ivf_stmask_axis_weights(int n_out, int n_in, float sigma, float* A_host);
/* M = A_H S A_W^T per (b,t): tmp[i][x] = sum_j S[i,j] A_W[x,j] (j ascending), M[y,x] = sum_i A_H[y,i] tmp[i][x]
 * (i ascending).  A_H [H,gh], A_W [W,gw] on the device.  Any non-negative matrices do: H = W = 1 with the uniform
 * rows A_H = 1/gh, A_W = 1/gw gives the spatial mean of S per frame, which is how the record's time_mask is made
 * (ivf_search.MaskSearch._run_spacetime). */
int ivf_stmask_expand_fwd(const float* S, const float* A_H, const float* A_W, float* M, int B, int T, int gh, int gw,
                          int H, int W, ivf_stream_t stream);
/* The exact adjoint, dS = A_H^T dM A_W, one pass over dM, one workgroup per (b,t). */
int ivf_stmask_expand_bwd(const float* dM, const float* A_H, const float* A_W, float* dS, int B, int T, int gh, int gw,
                          int H, int W, ivf_stream_t stream);
/* Per-pixel freeze: x [B,C,T,HW] NCTHW, M [B,T,HW] in [0,1]; p as ivf_freeze_fwd names it (out_cpad 0 NCTHW, else
 * channels-last rows of out_cpad >= C floats, pad lanes +0.0; 4 needs C <= 4).  The arithmetic and its order are
 * those of ivf_freeze_fwd: a spatially constant M gives the same bits. */
int ivf_stfreeze_fwd(const float* x, const float* M, float* p, int B, int C, int T, int HW, int out_cpad,
                     ivf_stream_t stream);
/* dM[b,u,px] = sum_c (P[u-1] - X[u]) G[u], c ascending, G the reverse scan of g (layout as ivf_freeze_bwd's g_cpad;
 * pad lanes ignored); dM[:,0] = 0.0 exactly.  T <= 64.  No reduction across pixels, no workspace. */
int ivf_stfreeze_bwd(const float* x, const float* M, const float* g, float* dM, int B, int C, int T, int HW, int g_cpad,
                     ivf_stream_t stream);
/* Regulariser: sig = sigmoid(raw); terms[b] = {lam1 sum S, lam2 TVt, lam3 TVs} / (gh gw) with
 * TVt = sum_cells sum_{u=1}^{T-2} |S[u-1]-S[u]|^3 + |S[u+1]-S[u]|^3 (calc_tv_norm's `val`, mask.py:93-96, per cell,
 * without its (.^(1/3))^3 chain: the identity in value, NaN in gradient at 0) and TVs the same cube over vertical and
 * horizontal neighbours within a frame; dreg_dsig = d(sum of the three)/dsig.  One workgroup per clip. */
int ivf_stmask_reg(const float* raw, int B, int T, int gh, int gw, float lam1, float lam2, float lam3, float* sig,
                   float* terms, float* dreg_dsig, ivf_stream_t stream);
/* Loop tail: traj_row[b] = (J, l1, tvt, tvs, score), J = l1 + tvt + tvs + score; chain through the sigmoid and the
 * Adam step of ivf_search_step / ivf_adam_step on raw [B,T,gh,gw]. */
int ivf_stmask_step(float* raw, const float* sig, const float* dscore_dsig, const float* dreg_dsig, const float* terms,
                    const float* score, float* exp_avg, float* exp_avg_sq, float* traj_row, int B, int T, int gh, int gw,
                    int step, float lr, float beta1, float beta2, float eps, ivf_stream_t stream);
/* Bytes of caller-owned scratch of ivf_{i3d,clstm}_stsearch for b = B clips (M, dM, sig, dreg, dsig, terms, score);
 * 0 with the message set for a shape the loop refuses. */
size_t ivf_stsearch_workspace_bytes(int B, int T, int H, int W, int gh, int gw);

/* ------------------------------------------------------------------ Integrated Gradients for video (csrc/ig_ops.hip)
 * An EXTENSION with no counterpart in the reference.  Path x(alpha) = x0 + alpha (x - x0) from a baseline
 * clip x0 to the clip x [b,C,T,HW]; nodes alpha [K] and weights w [K] are device arrays (any quadrature rule).
 * base_kind: 0 'frozen' (x0 = frame 0 of the row's own clip at every frame, mask.py:123-128), 1 'constant' (base_value
 * everywhere), 2 'clip' (base [b,C,T,HW]); base is read for kind 2 only.  The (clip, node) rows are numbered
 * g = clip * K + k.  No float atomics; every sum has a fixed order, so a clip's results depend neither on the batch it
 * ran in nor on how the rows were cut into windows.
 *
 * ivf_ig_stage: rows [first, first+count) into out; row j is clip (first+j)/K at node (first+j)%K, each element
 * fmaf(alpha, x - x0, x0): exact where x == x0 and at alpha == 0.  layout as the mask kernels name it: 0 NCTHW
 * [count,C,T,HW], 4 16-byte channels-last pixels [count,T,HW,4] (C <= 4, pad lanes written +0.0). */
int ivf_ig_stage(const float* x, int base_kind, const float* base, float base_value, const float* alpha, int b, int C,
                 int T, int HW, int K, long long first, int count, float* out, int layout, ivf_stream_t stream);
/* Gsum [b,C,T,HW] (NCTHW, zeroed by the caller once per call) += the window's rows of din (layout as above, row j the
 * gradient of row first+j): per element acc = fmaf(w[k], g, acc) over the window's rows of its clip, k ascending.  Pad
 * lanes of din are never read into a result. */
int ivf_ig_accumulate(const float* din, int layout, const float* w, int K, long long first, int count, float* Gsum, int b,
                      int C, int T, int HW, ivf_stream_t stream);
/* A = (x - x0) Gsum; ig_map [b,T,HW] = sum_c A (c ascending); frames [b,T] = sum_px ig_map and abs_frames [b,T] =
 * sum_px sum_c |A| (thread-order partial sums, a wave64 shuffle tree, then the waves in order); total [b] = sum_t
 * frames (t ascending). */
int ivf_ig_finish(const float* x, int base_kind, const float* base, float base_value, const float* Gsum, int b, int C,
                  int T, int HW, float* ig_map, float* frames, float* abs_frames, float* total, ivf_stream_t stream);
/* Bytes of caller-owned scratch of ivf_{i3d,clstm}_ig for b clips and K nodes (Gsum, the per-row targets, the row
 * scores); 0 with the message set for bad dims. */
size_t ivf_ig_workspace_bytes(int b, int C, int T, int HW, int K);

/* ------------------------------------------------------------------ exhaustive one-box search (maskType 'stcombi')
 * The gradient-free counterpart of 'spacetime', as 'combi' is of the temporal gradient search; an extension as well.
 * A candidate (a, L, i0, bh, j0, bw) is the binary S that is 1 on frames [a, a+L), grid rows [i0, i0+bh) and grid
 * columns [j0, j0+bw): one temporal blob times one rectangle of cells, L <= max_len, bh <= mh, bw <= mw.  The three axes
 * are three one-blob tables in the order of ivf_blob_count (length ascending, then start);
 * k = (kt n_h + kh) n_w + kw, n = n_t n_h n_w with n_t = ivf_blob_count(T, max_len), n_h = ivf_blob_count(gh, mh),
 * n_w = ivf_blob_count(gw, mw).
 * ivf_box_count: HOST.  n, or -1 (message set) unless 1 <= max_len <= T <= 64, 1 <= mh <= gh <= 32,
 * 1 <= mw <= gw <= 32. */
long long ivf_box_count(int T, int max_len, int gh, int gw, int mh, int mw);
/* Rows [first, first+count) of the flattened (clip, candidate) list of b clips x [b,C,T,H,W] into p; row j is clip
 * (first+j)/n, candidate (first+j)%n; count <= 65535.  out_cpad as ivf_blob_stage: 0 NCTHW [count,C,T,HW], 4 16-byte
 * channels-last pixels [count,T,HW,4] (C <= 4, pad lanes +0.0).  A_H [H,gh], A_W [W,gw] on the device.  The rows equal
 * (==) what ivf_stmask_expand_fwd followed by ivf_stfreeze_fwd write for the candidate's binary S; neither S nor M is
 * ever in memory. */
int ivf_box_stage(const float* x, int b, int C, int T, int H, int W, const float* A_H, const float* A_W, int gh, int gw,
                  int max_len, int mh, int mw, long long first, int count, float* p, int out_cpad, ivf_stream_t stream);
/* Selection over a score grid scores [b,n], one workgroup per clip.
 * J_k = (lam1 L bh bw + lam2 TVt_k + lam3 TVs_k) / (gh gw) + s_k, TVt and TVs those of ivf_stmask_reg on the binary S
 * (closed form; the same fp32 expressions and order as the spacetime loop's trajectory row).  best [b,6] =
 * (a, L, i0, bh, j0, bw) of argmin J (NaN skipped, the smaller k on a tie, all -1 if every score is NaN); best_obj [b]
 * and obj [b,n] optional; minimal [b,6] (optional): the smallest volume L bh bw with some
 * r = (orig - s) / (orig - full) >= threshold, the largest r within it, then the smaller k; all -1 if none. */
int ivf_box_select(const float* scores, const float* orig, const float* full, int b, int T, int gh, int gw, int max_len,
                   int mh, int mw, float lam1, float lam2, float lam3, float threshold, int* best, float* best_obj,
                   float* obj, int* minimal, ivf_stream_t stream);
/* Occlusion map from the score grid: drop [b,T,gh,gw], drop[b,t,i,j] = mean of (orig[b] - s_k) over the candidates
 * whose box covers cell (t,i,j), summed in ascending k; NaN scores are neither summed nor counted (NaN where none is
 * left).  One thread per cell, which visits the covering candidates only. */
int ivf_box_drop(const float* scores, const float* orig, int b, int T, int gh, int gw, int max_len, int mh, int mw,
                 float* drop, ivf_stream_t stream);

/* ------------------------------------------------------------------ RISE random-mask saliency (csrc/rise_ops.hip)
 * An EXTENSION with no counterpart in the reference (Petsiuk et al. 2018): n random coarse masks, one
 * forward each, a cell's importance = the mean score drop over the masks that froze it.  A mask lives on a grid
 * (gt, gh, gw), 1 <= gt <= T <= 64, 1 <= gh, gw <= 32; frame u belongs to temporal cell kt = (u gt) / T, cell
 * c = (kt gh + i) gw + j.  Mask k is the same for every clip; it freezes cell c iff
 *   fmix32( fmix32(seed + 0x9E3779B9 (k + 1)) ^ (0x85EBCA77 (c + 1)) ) < thresh          (uint32, wrapping;
 *   fmix32(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16)
 * with thresh = floor(p 2^32) computed by the caller, 0 refused.  No entry stores the masks: the bits are regenerated.
 *
 * Explicit bits of masks [first_k, first_k+count) as 0.0 / 1.0 into S [count,gt,gh,gw]. */
int ivf_rise_masks(unsigned seed, unsigned thresh, int first_k, int count, int gt, int gh, int gw, float* S,
                   ivf_stream_t stream);
/* Rows [first, first+count) of the flattened (clip, mask) list of b clips x [b,C,T,H,W] into p; row j is clip
 * (first+j)/n under mask (first+j)%n; count <= 65535.  out_cpad as the box staging entry: 0 NCTHW [count,C,T,HW], 4 16-byte
 * channels-last pixels [count,T,HW,4] (C <= 4, pad lanes +0.0, p 16-byte aligned).  A_H [H,gh], A_W [W,gw] on the
 * device, finite and non-negative.  The rows equal (==) what ivf_stmask_expand_fwd followed by ivf_stfreeze_fwd write
 * for the row's explicit per-frame S (S[u] = S_k[kt(u)]); neither S nor M is ever in memory. */
int ivf_rise_stage(const float* x, int b, int C, int T, int H, int W, const float* A_H, const float* A_W, int gt, int gh,
                   int gw, int n, unsigned seed, unsigned thresh, long long first, int count, float* p, int out_cpad,
                   ivf_stream_t stream);
/* The estimator from scores [b,n] and orig [b], d_k = orig - s_k, k ascending in plain fp32 adds, one thread per
 * (clip, cell), no atomics: cells [b,gt,gh,gw] = sum of d_k over the masks that froze the cell / count, count (int)
 * their number; a NaN score is neither summed nor counted; cells is NaN where count == 0.  mean_drop [b] = the mean of
 * d_k over the clip's non-NaN scores. */
int ivf_rise_reduce(const float* scores, const float* orig, int b, int n, unsigned seed, unsigned thresh, int gt, int gh,
                    int gw, float* cells, int* count, float* mean_drop, ivf_stream_t stream);

/* ------------------------------------------------------------------ Shapley value sampling (csrc/shapley_ops.hip)
 * An EXTENSION with no counterpart in the reference (Castro et al. 2009, Strumbelj & Kononenko 2014): the
 * players are the P = gt gh gw cells of a grid as in the RISE section above (1 <= gt <= T <= 64, 1 <= gh, gw <= 32, and
 * P <= 4096), a coalition is the set of frozen cells, its value the class score of the clip frozen per pixel by that
 * binary mask.  Permutation k freezes the cells one after another in the order of
 *   rank_k[c] = #{c' : (h(seed,k,c'), c') < (h(seed,k,c), c)},     h = the hash of the RISE section (lexicographic
 *   order: a hash tie falls to the lower cell index, so every row is a permutation of 0 .. P-1),
 * and with antithetic = 1 an odd k is permutation k-1 (hashed as itself) reversed: rank_k[c] = P-1 - rank_{k-1}[c].
 * Row j = 0 .. P of permutation k freezes the cells with rank_k[c] < j: row 0 is the clip, row P the fully frozen clip.
 * The marginal of cell c is d_k[c] = s[k][rank_k[c]] - s[k][rank_k[c]+1] (> 0: freezing c lowers the score), and
 * sum_c d_k[c] = s[k][0] - s[k][P] for every k.  The permutations are the same for every clip.
 *
 * Rank table of permutations [first_k, first_k+count) into ranks [count,P] (uint16; antithetic 0 or 1). */
int ivf_shap_ranks(unsigned seed, int antithetic, int first_k, int count, int gt, int gh, int gw, unsigned short* ranks,
                   ivf_stream_t stream);
/* Rows [first, first+count) of the flattened (clip, permutation, prefix) list of b clips x [b,C,T,H,W] into p: row r is
 * clip r / (n (P+1)), permutation (r / (P+1)) % n, prefix r % (P+1), of the n (P+1) rows a clip has; count <= 65535.
 * ranks [n,P] on the device: the table of permutations 0 .. n-1 (ivf_shap_ranks, or the caller's own).  out_cpad, A_H,
 * A_W as ivf_rise_stage.  The rows equal (==) what ivf_stmask_expand_fwd followed by ivf_stfreeze_fwd write for the
 * row's explicit per-frame S (S[u][c] = 1 iff rank[c] < prefix, c in the temporal cell of frame u); neither S nor M is
 * ever in memory. */
int ivf_shap_stage(const float* x, int b, int C, int T, int H, int W, const float* A_H, const float* A_W, int gt, int gh,
                   int gw, int n, const unsigned short* ranks, long long first, int count, float* p, int out_cpad,
                   ivf_stream_t stream);
/* The estimator from scores [b,n,P+1] and ranks [n,P], k ascending in plain fp32, one thread per (clip, cell), no
 * atomics: cells [b,gt,gh,gw] = sum_k d_k / count, count (int) the number of terms; a term with a NaN score on either
 * side (or a rank outside 0 .. P-1) is neither summed nor counted; cells is NaN where count == 0.  std_err = sqrt(sum_k
 * (d_k - cells)^2 / (count - 1) / count), a second pass in the same order, NaN where count < 2.  total [b] = the mean of
 * s[k][0] - s[k][P] over the permutations whose two end scores are finite (NaN if none): what the cells sum to. */
int ivf_shap_reduce(const float* scores, const unsigned short* ranks, int b, int n, int gt, int gh, int gw, float* cells,
                    float* std_err, int* count, float* total, ivf_stream_t stream);

/* ------------------------------------------------------------------ deletion / insertion curves (csrc/curve_ops.hip)
 * An EXTENSION with no counterpart in the reference (Petsiuk et al. 2018): the faithfulness measure that
 * compares the attribution methods.  The players are the P = gt gh gw cells of a grid as in the Shapley section above
 * (1 <= gt <= T <= 64, 1 <= gh, gw <= 32, P <= 4096); an attribution (higher = more important) ranks them per clip, and
 * with J = ceil(P / step), k_j = min(j step, P), j = 0 .. J:
 *   deletion row j : cell c frozen iff rank[c] <  k_j   (row 0 the clip, row J the fully frozen clip)
 *   insertion row j: cell c frozen iff rank[c] >= k_j   (row 0 the fully frozen clip, row J the clip)
 * curves is a bitmask, 1 deletion, 2 insertion, 3 both (deletion first); a clip has ncurves (J+1) rows, flattened as
 * [clip][curve][j].
 *
 * Rank table [b,P] (uint16) of a [b,t_in,gh,gw], t_in == gt or t_in == T (then a grid cell is the mean over the frames
 * u of its temporal cell (u gt) / T: the fp32 sum in ascending u, one division by the frame count).  order 0:
 *   rank[c] = #{c' : a[c'] > a[c], or a[c'] == a[c] and c' < c};       order 1 flips > to <.
 * A NaN cell ranks after every number in either order, NaN cells among themselves by index; -0.0 == +0.0 is a tie. */
int ivf_curve_ranks(const float* a, int b, int t_in, int T, int gt, int gh, int gw, int order, unsigned short* ranks,
                    ivf_stream_t stream);
/* Rows [first, first+count) of the flattened (clip, curve, j) list of b clips x [b,C,T,H,W] into p; count <= 65535.
 * ranks [b,P] on the device: one table per clip (ivf_curve_ranks, or the caller's own).  out_cpad, A_H, A_W as
 * ivf_shap_stage.  The rows equal (==) what ivf_stmask_expand_fwd followed by ivf_stfreeze_fwd write for the row's
 * explicit per-frame binary S; neither S nor M is ever in memory. */
int ivf_curve_stage(const float* x, int b, int C, int T, int H, int W, const float* A_H, const float* A_W, int gt, int gh,
                    int gw, const unsigned short* ranks, int curves, int step, long long first, int count, float* p,
                    int out_cpad, ivf_stream_t stream);
/* From scores [b,ncurves,J+1] (ncurves = the curves named by the bitmask), one thread per (clip, curve), plain fp32 in
 * ascending j, integer widths, one final division, no atomics:
 *   auc [b,ncurves]      = (1 / (2P)) sum_{j<J} (k_{j+1} - k_j) (s_j + s_{j+1})
 *   auc_norm [b,ncurves] = (auc - s_lo) / (s_hi - s_lo),  s_hi the score of the clip, s_lo of the fully frozen clip (the
 *                          curve's own end rows), NaN where they are equal.
 * Any NaN score in a curve makes both of its outputs NaN. */
int ivf_curve_reduce(const float* scores, int b, int ncurves, int curves, int P, int step, float* auc, float* auc_norm,
                     ivf_stream_t stream);

/* ------------------------------------------------------------------ linear surrogates: KernelSHAP and LIME (csrc/linsur_ops.hip)
 * An EXTENSION with no counterpart in the reference (Lundberg & Lee 2017, Ribeiro et al. 2016): a linear
 * model of the score drop in the frozen cells, fitted by least squares in fp64 on the device.  The players are the
 * P = gt gh gw cells of a grid as in the Shapley section above, 2 <= P <= 1024.  z_kc = 1: sample row k freezes cell c.
 * The n sample rows are the same for every clip and are kept as packed bits, bits [n, ceil(P/32)] (uint32): bit c % 32
 * of word c / 32 holds z_kc, the unused high bits are zero.  A clip has the n sample rows and one further row n with
 * every cell frozen: scores [b,n+1].  The fitted quantity is y_bk = (double)score_x[b] - (double)scores[b,k], so that a
 * cell's coefficient is > 0 where freezing it lowers the score.
 *
 * KernelSHAP rows [first_k, first_k+count): with h the hash and rank_k the table of the Shapley section,
 *   s_k = 1 + #{i : h(seed, base_k, P) >= size_table[i]},  size_table [P-2] (uint32) the caller's: floor(2^32 CDF(i)),
 *   i = 1 .. P-2, of q(s) ~ 1 / (s (P-s)) on 1 .. P-1 (the Shapley kernel's size distribution; may be null at P = 2),
 * and row k freezes the cells with rank_k[c] < s_k.  paired = 1: an odd k is the complement of row k-1 (base_k = k-1,
 * the rank reversed, s_k = P - s_{k-1}); else base_k = k.  sizes [count] (uint16) = s_k. */
int ivf_kshap_rows(unsigned seed, int paired, int first_k, int count, int gt, int gh, int gw, const unsigned* size_table,
                   unsigned* bits, unsigned short* sizes, ivf_stream_t stream);
/* LIME rows [first_k, first_k+count): bit c of row k = h(seed, k, c) < thresh, the bits of ivf_rise_masks. */
int ivf_lime_rows(unsigned seed, unsigned thresh, int first_k, int count, int gt, int gh, int gw, unsigned* bits,
                  ivf_stream_t stream);
/* Rows [first, first+count) of the flattened (clip, row) list of b clips x [b,C,T,H,W] into p: row r is clip r / (n+1)
 * under sample row r % (n+1) of bits [n, ceil(P/32)], row n every cell frozen; count <= 65535.  out_cpad, A_H, A_W as
 * ivf_rise_stage.  The rows equal (==) what ivf_stmask_expand_fwd followed by ivf_stfreeze_fwd write for the row's
 * explicit per-frame S; neither S nor M is ever in memory. */
int ivf_lin_stage(const float* x, int b, int C, int T, int H, int W, const float* A_H, const float* A_W, int gt, int gh,
                  int gw, int n, const unsigned* bits, long long first, int count, float* p, int out_cpad,
                  ivf_stream_t stream);
/* The fp64 moments of the weighted least-squares problem from scores [b,n+1], score_x [b] and bits [n, ceil(P/32)]
 * (here 1 <= P <= 1024), every element one chain in ascending k, products rounded before they are added, no atomics:
 *   w_k = wtab[popcount(row k)] (wtab [P+1] fp64 on the device; null: w_k = 1) -> wrow [n]
 *   N [P,P] = sum_k w_k [z_kc & z_kc'],  v [P] = sum_k w_k z_kc,  Wsum [1] = sum_k w_k,
 *   r [b,P] = sum_k fl(w_k y_bk) z_kc,   t [b] = sum_k fl(w_k y_bk),
 * a row that does not set a bit adds nothing.  ok [b] (int) = 0 where score_x[b] or any of the clip's n+1 scores is
 * not finite, else 1.  All outputs are the caller's. */
int ivf_lin_moments(const float* scores, const float* score_x, const unsigned* bits, const double* wtab, int b, int n,
                    int P, double* N, double* v, double* Wsum, double* r, double* t, double* wrow, int* ok,
                    ivf_stream_t stream);
/* Bytes of the caller's factor workspace of ivf_lin_solve for P players; 0 with the message set for a bad P. */
size_t ivf_lin_workspace_bytes(int P);
/* The fit from the moments.  kind 0, KernelSHAP (2 <= P): the efficiency constraint sum_c phi_c = total_b =
 * score_x[b] - scores[b,n] eliminated through the last cell l = P-1, m = P-1 unknowns,
 *   A[c,c'] = N[c,c'] - N[c,l] - N[l,c'] + N[l,l],   rhs[b,c] = (r[b,c] - r[b,l]) - total_b (N[c,l] - N[l,l]),
 *   phi_l = total_b - sum_{c<l} phi_c (ascending c, fp64), intercept 0.
 * kind 1, LIME (1 <= P): the weighted ridge regression with a free intercept, m = P unknowns, mu = v / Wsum,
 *   G[c,c'] = N[c,c'] - Wsum (mu_c mu_c') + ridge [c == c'],   rhs[b,c] = r[b,c] - mu_c t_b,
 *   intercept[b] = t_b / Wsum - sum_c mu_c phi_c (ascending c, fp64).
 * The system is factored once by a blocked right-looking Cholesky in fp64 (fixed summation order, no atomics) and
 * solved for the b right-hand sides.  A pivot d_j <= 2^-20 A_jj (A_jj the entry before the factorisation) or a pivot
 * that is not finite marks the system singular: ok = 0 and NaN cells for EVERY clip.  ok [b] is in/out (ivf_lin_moments
 * wrote it): a clip with ok == 0 gets NaN cells and intercept.  cells [b,P] and intercept [b] are fp32, each the
 * fp64 solution rounded once; total [b] = (float)total_b.  work: ivf_lin_workspace_bytes(P) bytes, 8-byte aligned. */
int ivf_lin_solve(int kind, const double* N, const double* v, const double* Wsum, const double* r, const double* t,
                  const float* scores, const float* score_x, int b, int n, int P, double ridge, void* work, float* cells,
                  float* intercept, float* total, int* ok, ivf_stream_t stream);
/* Fit quality r2 [b] = 1 - sum_k w_k (y_bk - yhat_bk)^2 / sum_k w_k (y_bk - t_b / Wsum)^2, yhat_bk = intercept[b] +
 * sum_c cells[b,c] z_kc (ascending c) from the fp32 outputs widened to fp64 (intercept null: 0), wrow [n] as
 * ivf_lin_moments wrote it (null: 1); each sum one chain in ascending k.  NaN where the denominator is 0 or
 * ok[b] == 0. */
int ivf_lin_fit(const float* scores, const float* score_x, const unsigned* bits, const double* wrow, const float* cells,
                const float* intercept, const double* t, const double* Wsum, const int* ok, int b, int n, int P, float* r2,
                ivf_stream_t stream);

/* ------------------------------------------------------------------ SmoothGrad, SmoothGrad^2, VarGrad (csrc/smoothgrad_ops.hip)
 * An EXTENSION with no counterpart in the reference (Smilkov et al. 2017, Hooker et al. 2019): n noisy
 * samples x + sigma z_k of a clip x [b,C,T,HW], one forward and backward each, and per input element the first two
 * moments of g = d score / d input over the samples.  The (clip, sample) rows are numbered g = clip * n + k.
 * Noise: one standard normal per sample k and element e = (c T + t) HW + px (the NCTHW index inside ONE clip, so it is
 * the same for every clip and either staged layout), C T HW <= 2^31 - 1, all hash arithmetic uint32 and wrapping, fmix32
 * as in the RISE section above:
 *   key = fmix32(seed + 0x9E3779B9 (k + 1));  a = fmix32(key ^ (0x85EBCA77 (e + 1)));  h2 = fmix32(a + 0x9E3779B9)
 *   u1 = (2 (a >> 9) + 1) 2^-24 in (0,1);  u2 = (h2 >> 8) 2^-24 in [0,1)          (both exact in fp32)
 *   z = sqrtf(-2 logf(u1)) * cospif(2 u2),  |z| <= sqrt(48 ln 2) = 5.768
 * one hash pair per element, no sin / cos pairing.  No entry stores the noise: it is regenerated.  No float atomics;
 * every sum has a fixed order, so a clip's results depend neither on the batch it ran in nor on how the rows were cut
 * into windows.
 *
 * Explicit z of samples [first_k, first_k + count) into z_out [count,C,T,HW]. */
int ivf_sg_noise(unsigned seed, int first_k, int count, int C, int T, int HW, float* z_out, ivf_stream_t stream);
/* sigma_out [b] = level * (max(x_clip) - min(x_clip)), one fp32 subtraction and one fp32 multiplication, computed on the
 * device; level finite and >= 0; a NaN element is skipped by the min and the max. */
int ivf_sg_range(const float* x, int b, int C, int T, int HW, float level, float* sigma_out, ivf_stream_t stream);
/* Rows [first, first+count) into out; row j is clip (first+j)/n at sample (first+j)%n, each element
 * fmaf(sigma[clip], z, x): equal to x where sigma == 0 (x == -0.0 becomes +0.0).  layout as the mask kernels name it: 0
 * NCTHW [count,C,T,HW] (16-byte accesses when HW % 4 == 0 and x, out are 16-byte aligned), 4 16-byte channels-last pixels
 * [count,T,HW,4] (C <= 4, out 16-byte aligned, pad lanes written +0.0). */
int ivf_sg_stage(const float* x, const float* sigma, int b, int C, int T, int HW, int n, unsigned seed, long long first,
                 int count, float* out, int layout, ivf_stream_t stream);
/* G1, G2 [b,C,T,HW] (NCTHW, zeroed by the caller once per call) += the window's rows of din (layout as above, row j the
 * gradient of row first+j): per element G1 = G1 + g and G2 = fmaf(g, g, G2) over the window's rows of its clip, k
 * ascending, din read once for both.  Pad lanes of din are never read into a result. */
int ivf_sg_accumulate(const float* din, int layout, int n, long long first, int count, float* G1, float* G2, int b, int C,
                      int T, int HW, ivf_stream_t stream);
/* Every operation rounded once in the order written, c ascending from +0.0:
 *   sg_map [b,T,HW] = sum_c |G1 / n|;  sq_map = sum_c G2 / n;  var_map = sum_c (G2 - G1 * (G1 / n)) / (n - 1), 0.0 at n == 1
 * sg_frames, sq_frames, var_frames [b,T] = sum_px of each map in the order of ivf_ig_finish (thread-order partial sums, a
 * wave64 shuffle tree, then the waves in order).  n <= 2^24.  var_map cancels where the gradient hardly moves under
 * the noise and may come out slightly negative there; nothing is clamped. */
int ivf_sg_finish(const float* G1, const float* G2, int n, int b, int C, int T, int HW, float* sg_map, float* sq_map,
                  float* var_map, float* sg_frames, float* sq_frames, float* var_frames, ivf_stream_t stream);
/* Bytes of caller-owned scratch of ivf_{i3d,clstm}_smoothgrad for b clips and n samples: G1, G2 (b C T HW floats each),
 * sigma (b floats), the per-row targets (b n ints), the row scores (b n floats), in that order, each piece rounded up to
 * 256 bytes; 0 with the message set for bad dims. */
size_t ivf_sg_workspace_bytes(int b, int C, int T, int HW, int n);

/* ------------------------------------------------------------------ Score-CAM for video (csrc/scorecam_ops.hip)
 * An EXTENSION with no counterpart in the reference (Wang et al., CVPR-W 2020): the activation-map method
 * that uses no gradient.  Per clip a target layer gives channel-major activations A [nc,gt,gh,gw], cells = gt gh gw <=
 * 8192, 1 <= gt <= T <= 64, 1 <= gh, gw <= 32; frame u belongs to temporal cell kt = (u gt) / T as in the RISE section.
 *   normalise  lo = min A_k, hi = max A_k; valid = lo, hi finite and hi > lo; the freeze plane
 *              F_k = (hi - A_k) / (hi - lo) in fp32 (one subtraction per operand pair, one correctly rounded division),
 *              F_k == 1 where the channel is not valid: 0 where the channel fires most, 1 where it is silent.
 *   stage      a clip has nc + 1 rows.  Row r < nc: M[u] = A_H F_r[kt(u)] A_W^T summed and rounded as
 *              ivf_stmask_expand_fwd does, then perturb 0 ('freeze'): P[0] = X[0], P[u] = (1 - M) X[u] + M P[u-1]
 *              (ivf_stfreeze_fwd's expression), perturb 1 ('blank'): P[u] = (1 - M) X[u] for every u.  Row nc is the
 *              baseline row, M == 1 exactly: every frame is frame 0 ('freeze'), +0.0 everywhere ('blank').
 *   reduce     d_k = s_k - s_nc; a channel counts when it is valid and d_k is not NaN, any other has w_k = 0.
 *              weights_kind 0 ('increase'): w_k = d_k.  1 ('softmax'): w_k = expf(d_k - d_max) / sum, d_max and the sum
 *              (k ascending) over the counting channels.  cam[p] = max(sum_k w_k A[k,p], 0), k ascending, a multiply
 *              and an add each, channels of weight 0 left out.
 * No atomics; every sum has a fixed order, so a clip's numbers depend neither on the batch nor on the chunking.
 *
 * A [b,nc,cells] -> lo, hi [b,nc] (a zero as +0.0; NaN if the plane holds one), valid [b,nc] (int 0 / 1), F [b,nc,cells]. */
int ivf_scorecam_normalise(const float* A, int b, int nc, int cells, float* lo, float* hi, int* valid, float* F,
                           ivf_stream_t stream);
/* Rows [first, first+count) of the flattened (clip, row) list of b clips x [b,C,T,H,W] into p; row j is clip
 * (first+j)/(nc+1), row (first+j)%(nc+1) of it; count <= 65535.  F [b,nc,gt,gh,gw] in [0, 1]; out_cpad, A_H, A_W as
 * ivf_rise_stage.  Under perturb 0 the rows r < nc equal (==) what ivf_stmask_expand_fwd followed by ivf_stfreeze_fwd
 * write for the row's explicit per-frame S (S[u] = F_r[kt(u)]); neither S nor M is ever in memory. */
int ivf_scorecam_stage(const float* x, int b, int C, int T, int H, int W, const float* A_H, const float* A_W, int gt,
                       int gh, int gw, const float* F, int nc, int perturb, long long first, int count, float* p,
                       int out_cpad, ivf_stream_t stream);
/* scores [b,nc+1], A [b,nc,cells], valid [b,nc] -> weights_out [b,nc], cam_out [b,cells]. */
int ivf_scorecam_reduce(const float* scores, const float* A, const int* valid, int b, int nc, int cells, int weights_kind,
                        float* weights_out, float* cam_out, ivf_stream_t stream);

/* Clip ingest: the arithmetic of ImLoader.__getitem__ /
 * KTHImLoader.__getitem__ after the JPEG decode (data_loader_jpg.py:29-37,
 * data_loader_kth.py:25-44): uint8 frames [B][T][H][W][C] -> float32 (exact), permuted to
 * [B][C][T][H][W] (layout IVF_INGEST_NCTHW, the tensor the reference hands to the model) or
 * to channels-last rows of cpad >= C floats with zero pad lanes (IVF_INGEST_CL, the plan's
 * input layout).  The host uploads a quarter of the bytes of the fp32 clip. */
#define IVF_INGEST_NCTHW 0
#define IVF_INGEST_CL 1
int ivf_clip_ingest_u8(const unsigned char* frames, float* out, int B, int T, int H, int W, int C, int layout,
                       int cpad, ivf_stream_t stream);

/* ------------------------------------------------------------------ Unit3D */

/* Arithmetic of the implicit-GEMM convolution:
 *  IVF_MATH_FP32    v_mfma_f32_32x32x2_f32: exact fp32 FMA chains (157 TFLOP/s peak);
 *  IVF_MATH_BF16X3  every operand split x = hi + lo (two bf16), three
 *                   v_mfma_f32_32x32x16_bf16 per k-step (lo*hi + hi*lo + hi*hi), fp32
 *                   accumulate: ~2^-17 relative per product, 5.3x the fp32-MFMA rate;
 *  IVF_MATH_BF16X6  every operand split x = hi + mid + lo (three bf16 = all 24 bits of the fp32
 *                   significand), six MFMAs per k-step (every term down to 2^-16 of the product), fp32
 *                   accumulate: an fp32 product to ~2^-23 -- the reference's fp32 arithmetic on the bf16
 *                   matrix cores, 2.65x the fp32-MFMA rate (ceiling 417 TFLOP/s);
 *  IVF_MATH_BF16ACT activations AND gradients are stored as bf16 in HBM (round-to-nearest-even in the
 *                   epilogues), weights stay split hi/lo, two MFMAs per k-step (a*lo + a*hi), fp32
 *                   accumulate (BASELINE configs[4]: "bf16 activations").  In this mode every in / out /
 *                   in2 / out2 / relu_mask pointer of ivf_conv3d addresses bf16 elements (same element
 *                   offsets), with two exceptions at the ends of the network: a 4-channel-pixel strided
 *                   convolution (IVF_CONV_PIX4, the stem) READS fp32 pixels, and a depth-to-space
 *                   backward (d2s, the stem's input gradient) WRITES fp32. */
#define IVF_MATH_FP32 0
#define IVF_MATH_BF16X3 1
#define IVF_MATH_BF16X6 2
#define IVF_MATH_BF16ACT 3

/* One convolution as implicit GEMM on the matrix cores.  Forward of Unit3D
 * (models/I3D_doubled.py:83-118: asymmetric zero pad + Conv3d + BN(eval) + ReLU) and,
 * with the packed backward weights, its backward-data.  Channels-last in/out. */
typedef struct {
  int B, Ti, Hi, Wi;           /* input positions */
  int Cin, in_ld, in_coff;     /* channel window read (Cin % 4 == 0) */
  int To, Ho, Wo;              /* output positions (block grid when d2s) */
  int Cout, out_ld, out_coff;  /* rows of the packed weight / channel window written */
  int kT, kH, kW, sT, sH, sW;  /* kernel, stride */
  int pT, pH, pW;              /* FRONT zero padding; back padding is implied by To/Ho/Wo */
  int relu;                    /* max(.,0) in the epilogue */
  int accumulate;              /* out += result (before relu / mask) */
  int mask_ld, mask_coff;      /* geometry of relu_mask (same positions as out) */
  int d2s;                     /* depth-to-space output: stride-2 backward-data */
  int dT, dH, dW, dC;          /* d2s: real output dims and channels written */
  int bsT, bsH, bsW;           /* d2s: block strides (forward strides, 1 or 2) */
  int math;                    /* IVF_MATH_*; must match the weight pack */
  int variant;                 /* IVF_CONV_AUTO, or a kernel variant id from ivf_conv3d_variants() */
  /* optional second input of a 1x1x1 conv: GEMM-K channels [K0, Cin) are read from in2 (same
   * positions; row length in2_ld, channel offset in2_coff), channels [0, K0) from `in` */
  int K0, in2_ld, in2_coff;
  const float* in2;
  /* optional second OUTPUT window (forward epilogues only: no accumulate, no relu_mask, no d2s): columns
   * [N0, Cout) are written to out2 (row length out2_ld, channel offset out2_coff, column n - N0) instead of
   * `out` -- one GEMM for several units that read the same input and write different buffers (an Inception
   * module's b0 | b1a | b2a).  Served by the implicit-GEMM tiles only. */
  int N0, out2_ld, out2_coff;
  float* out2;
  /* 1-bit ReLU gates (1 byte per 8 channels, rows of gate_*_ld BYTES; channel offsets are multiples of 8 and so is
   * Cout / N0).  A forward epilogue can record (value > 0) of what it stores: gate_out for the `out` window,
   * gate_out2 for the `out2` window.  A backward epilogue can take its gate from such a record (gate_in) instead
   * of re-reading the fp32 activation through `relu_mask` -- 1/32 of the bytes.  All optional (null = off). */
  unsigned char* gate_out;
  unsigned char* gate_out2;
  const unsigned char* gate_in;
  int gate_out_ld, gate_out_coff, gate_out2_ld, gate_in_ld, gate_in_coff;
} ivf_conv3d_desc;

/* Kernel variants: the eight tile shapes of the plain implicit GEMM (IVF_CONV_IGEMM_BASE + 0..7: three
 * narrow tiles for every arithmetic mode, three wide and two small ones for the split-bf16 modes), the
 * 4-channel-pixel kernel (IVF_CONV_PIX4) and the tiles of the LDS-halo kernel (IVF_CONV_HALO_BASE + i;
 * split-bf16, stride 1, 2 <= k <= 4 only).  All variants compute the same sums; they differ in speed
 * per layer shape and (in the last bits) in summation order, so a plan fixes one variant per layer.
 * ivf_conv3d_variants lists the candidates for a descriptor (one that this shape or arithmetic mode
 * cannot run reports so when launched); ivf_conv3d_default_variant returns the id that IVF_CONV_AUTO
 * runs, or a negative error. */
#define IVF_CONV_AUTO 0
#define IVF_CONV_IGEMM_BASE 1
#define IVF_CONV_HALO_BASE 16
#define IVF_CONV_PIX4 15 /* 4-channel-pixel strided kernel (the stem): split-bf16, Cin = in_ld = 4, stride (1|2, 2, 2), k <= 7 */
int ivf_conv3d_variants(const ivf_conv3d_desc* d, int* ids, int max_ids);
int ivf_conv3d_default_variant(const ivf_conv3d_desc* d);

/* out = epilogue(conv(in, w_packed)): v = acc*scale[n] + shift[n] (NULL = 1 / 0);
 * relu_mask != NULL zeroes v where mask <= 0 (the ReLU below, for backward-data). */
int ivf_conv3d(const ivf_conv3d_desc* d, const float* in, const float* w_packed, const float* scale,
               const float* shift, const float* relu_mask, float* out, ivf_stream_t stream);

/* BatchNorm3d(eval) fold, I3D_doubled.py:75 (eps 1e-3). */
int ivf_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                float* scale, float* shift, int C, ivf_stream_t stream);

/* Reference weight [Cout][Cin][kT][kH][kW] -> forward pack [Cout][taps*CinPad]
 * (fp32, or bf16 planes with rows padded to 8: hi/lo for IVF_MATH_BF16X3 and IVF_MATH_BF16ACT, hi/mid/lo for
 * IVF_MATH_BF16X6);
 * w_packed holds ivf_conv3d_pack_fwd_elems() floats. */
size_t ivf_conv3d_pack_fwd_elems(int Cout, int CinPad, int kT, int kH, int kW, int math);
int ivf_conv3d_pack_fwd(const float* w_ref, float* w_packed, int Cout, int Cin, int CinPad, int kT,
                        int kH, int kW, int math, ivf_stream_t stream);
/* Same, as rows [row0, row0+Cout) of a packed matrix with rows_total rows: several units that
 * read the same input packed side by side so they run as one convolution. */
int ivf_conv3d_pack_fwd_rows(const float* w_ref, float* w_packed, int Cout, int Cin, int CinPad, int kT,
                             int kH, int kW, int row0, int rows_total, int math, ivf_stream_t stream);

/* Geometry of the backward-data convolution produced by ivf_conv3d_pack_bwd. */
typedef struct {
  int d2s;          /* 0: plain flipped conv (all strides 1); 1: depth-to-space form */
  int kT, kH, kW;   /* kernel of the backward conv over dY */
  int pT, pH, pW;   /* its front padding */
  int rows;         /* rows of the packed weight (= Cout of the backward conv) */
} ivf_conv3d_bwd_geom;

/* Backward-data pack, BN scale folded in: [rows][taps_b*Cout]; needs
 * rows*taps_b*Cout floats where taps_b = geom.kT*kH*kW (call with w_packed sized
 * by ivf_conv3d_pack_bwd_elems). */
size_t ivf_conv3d_pack_bwd_elems(int Cout, int CinPad, int kT, int kH, int kW, int sT, int sH, int sW,
                                 int pT, int pH, int pW, int math);
int ivf_conv3d_pack_bwd(const float* w_ref, const float* scale, float* w_packed, int Cout, int Cin,
                        int CinPad, int kT, int kH, int kW, int sT, int sH, int sW, int pT, int pH,
                        int pW, int math, ivf_conv3d_bwd_geom* geom, ivf_stream_t stream);

/* The 1x1x1 units b0 / b1a / b2a of an Inception module read the same input, so their
 * backward-data is ONE GEMM over the concatenated gradients [dY_b0 | dT_b1a | dT_b2a]:
 * pack unit by unit, in any order, into a [CinPad][Ktotal] matrix (column offset koff; the
 * unit ending at Ktotal also zeroes the row padding). */
size_t ivf_conv3d_pack_bwd_fused1x1_elems(int Ktotal, int CinPad, int math);
int ivf_conv3d_pack_bwd_fused1x1(const float* w_ref, const float* scale, float* w_packed, int Cout, int Cin,
                                 int CinPad, int koff, int Ktotal, int math, ivf_stream_t stream);

/* ------------------------------------------------------------------ pooling / head */

typedef struct {
  int B, Ti, Hi, Wi, C, in_ld, in_coff;
  int To, Ho, Wo, out_ld, out_coff;
  int kT, kH, kW, sT, sH, sW, pT, pH, pW; /* front ZERO padding (I3D_doubled.py:36-39) */
  /* forward only: record arg-max 255 ("no route") for windows whose maximum is not > 0.
   * When x is a ReLU output and the gradient is wanted below that ReLU, the backward then
   * needs no relu_mask: a cell with x <= 0 can only win a window whose maximum is <= 0. */
  int gate_nonpos;
  /* storage of x / y / dy / dx / relu_mask: 0 = float, 1 = bf16 (IVF_MATH_BF16ACT plans; same element offsets).  The
   * forward only selects, so it is exact in either storage; the backward sums in fp32 and rounds once on store. */
  int act_bf16;
} ivf_pool3d_desc;

/* MaxPool3dSamePadding.forward, I3D_doubled.py:15-40; argmax [positions_out][C] uint8
 * (flat tap of the winner, first strict maximum, pad cells count as 0). */
int ivf_maxpool3d_fwd(const ivf_pool3d_desc* d, const void* x, void* y, unsigned char* argmax,
                      ivf_stream_t stream);
int ivf_maxpool3d_bwd(const ivf_pool3d_desc* d, const void* dy, const unsigned char* argmax, void* dx,
                      const void* relu_mask, int accumulate, ivf_stream_t stream);

/* I3D head, I3D_doubled.py:360-380, for a pooling window covering the whole feature
 * map: feat [B,npos,C] -> pooled [B,C] (optional) -> logits [B,K] -> probs [B,K]
 * (softmax over K if softmax != 0, else a copy).  w is the reference
 * logits.conv3d.weight viewed as [K][C]. */
int ivf_head_fwd(const float* feat, const float* w, const float* bias, float* pooled, float* logits,
                 float* probs, int B, int npos, int C, int K, int softmax, ivf_stream_t stream);

/* Backward of the head.  Upstream gradient: dout [B,K] if non-NULL, else one-hot at
 * target[b].  score[b] = probs[b,target[b]] (optional, needs target).
 * dpooled [B,C] optional; dfeat [B,npos,C] optional, gated by feat > 0 when gate_relu. */
int ivf_head_bwd(const float* feat, const float* w, const float* probs, const int* target,
                 const float* dout, float* score, float* dpooled, float* dfeat, int B, int npos, int C,
                 int K, int softmax, int gate_relu, ivf_stream_t stream);
/* The same two with the feature map (and dfeat) stored as bf16 (IVF_MATH_BF16ACT plans); pooled / logits /
 * probs / score / dpooled stay fp32. */
int ivf_head_fwd_bf16(const void* feat, const float* w, const float* bias, float* pooled, float* logits,
                      float* probs, int B, int npos, int C, int K, int softmax, ivf_stream_t stream);
int ivf_head_bwd_bf16(const void* feat, const float* w, const float* probs, const int* target,
                      const float* dout, float* score, float* dpooled, void* dfeat, int B, int npos, int C,
                      int K, int softmax, int gate_relu, ivf_stream_t stream);

/* ------------------------------------------------------------------ Grad-CAM */

/* grad_cam_videos.py:98-110: weights[b,k] = mean_pos grad; cam[b,pos] = relu(sum_k w*feat). */
int ivf_gradcam_reduce(const float* feat, const float* grad, float* weights, float* cam, int B, int npos,
                       int C, ivf_stream_t stream);
/* feat and grad stored as bf16 (IVF_MATH_BF16ACT plans); weights and cam fp32. */
int ivf_gradcam_reduce_bf16(const void* feat, const void* grad, float* weights, float* cam, int B, int npos,
                            int C, ivf_stream_t stream);

/* The activation-map family around Grad-CAM (csrc/cam_ops.hip; a documented extension), from the same
 * two buffers: feat = A and grad = G, [B,npos,C] channels-last.  Per clip, s_k = sum_p A[p,k]:
 *   IVF_CAM_GRADCAM  w_k = mean_p G                                  cam[p] = relu(sum_k w_k A[p,k])
 *   IVF_CAM_PP       w_k = sum_p [G > 0] G / (2 + s_k G)             cam[p] = relu(sum_k w_k A[p,k])   (Grad-CAM++)
 *   IVF_CAM_XGRAD    w_k = (sum_p G A) / s_k, 0 where s_k == 0       cam[p] = relu(sum_k w_k A[p,k])   (XGrad-CAM)
 *   IVF_CAM_HIRES    w_k = 0 (none)                                  cam[p] = relu(sum_k G[p,k] A[p,k])
 *   IVF_CAM_LAYER    w_k = 0 (none)                                  cam[p] = relu(sum_k relu(G[p,k]) A[p,k])
 * kinds_host: n_kinds (1..5) distinct HOST ints; row i of weights [n_kinds,B,C] (optional) and of cam
 * [n_kinds,B,npos] belongs to kinds_host[i].  Kind 0 runs the kernels of ivf_gradcam_reduce (bit-equal to it).
 * No atomics, fixed summation order: a clip's rows depend neither on B, nor on its place in the batch, nor on the
 * other kinds of the call.  Non-finite values propagate as in Grad-CAM; the one guard is XGrad-CAM's s_k == 0.
 * The per-channel passes run over chunks of IVF_CAM_CHUNK positions; ws: ivf_cam_ws_bytes(B, npos, C) bytes. */
#define IVF_CAM_GRADCAM 0
#define IVF_CAM_PP 1
#define IVF_CAM_XGRAD 2
#define IVF_CAM_HIRES 3
#define IVF_CAM_LAYER 4
#define IVF_CAM_CHUNK 128
#define IVF_CAM_MAX_HID 256
size_t ivf_cam_ws_bytes(int B, int npos, int C);
int ivf_cam_reduce(const float* feat, const float* grad, int n_kinds, const int* kinds_host, float* weights,
                   float* cam, void* ws, int B, int npos, int C, ivf_stream_t stream);
/* feat and grad stored as bf16 (IVF_MATH_BF16ACT plans); weights and cam fp32. */
int ivf_cam_reduce_bf16(const void* feat, const void* grad, int n_kinds, const int* kinds_host, float* weights,
                        float* cam, void* ws, int B, int npos, int C, ivf_stream_t stream);

/* grad_cam_videos.py:113-138: per temporal slice bilinear resize (sh,sw)->(H,W)
 * (OpenCV INTER_LINEAR rule), repeat `step` frames, min/max normalise per slice block
 * (per_frame) or per clip.  cam [B,nslice,sh,sw] -> out [B,nslice*step,H,W];
 * minmax_ws: B*nslice*2 floats. */
int ivf_cam_resize_normalise(const float* cam, float* out, float* minmax_ws, int B, int nslice, int sh,
                             int sw, int H, int W, int step, int per_frame, ivf_stream_t stream);

/* ------------------------------------------------------------------ whole I3D */

typedef struct {
  int B;                 /* maximum clips per call */
  int C, T, H, W;        /* clip geometry, reference NCTHW */
  int num_classes;
  int stem_stride_t;     /* temporal stride of Conv3d_1a_7x7 (2, or last_stride) */
  int pool4a_stride_t;   /* MaxPool3d_4a_3x3 */
  int pool5a_stride_t;   /* MaxPool3d_5a_2x2 */
  int head_kt, head_kh, head_kw; /* AvgPool3d window: (2,7,7) / (finalTimeLength,4,5) */
  int softmax;           /* Model(softMax=...) */
  int math;              /* IVF_MATH_* for every Unit3D convolution (IVF_MATH_BF16ACT also selects bf16 storage of
                            every activation / gradient buffer of the plan except the clip and its gradient) */
} ivf_i3d_config;

typedef struct ivf_i3d ivf_i3d_t;

/* Host-side plan (shapes, buffer offsets, launch list).  No device work. */
int ivf_i3d_create(const ivf_i3d_config* cfg, ivf_i3d_t** out);
/* Run the HBM-bound branch of every Inception module (the 3x3x3 pool and b3b, both ways) on a side
 * stream beside the 3x3x3 convs of the other branches (fork at module entry, join before the next consumer, with
 * events inside every forward / backward call; results are bit-identical).  On by default (IVF_OVERLAP=0 in the
 * environment of ivf_i3d_create turns it off): +1.2 % measured, see DESIGN.md. */
int ivf_i3d_set_overlap(ivf_i3d_t* net, int on);
void ivf_i3d_destroy(ivf_i3d_t* net);
size_t ivf_i3d_weights_bytes(const ivf_i3d_t* net);
size_t ivf_i3d_workspace_bytes(const ivf_i3d_t* net);
/* Give the plan its two caller-owned device arenas (256-byte aligned). */
int ivf_i3d_bind(ivf_i3d_t* net, void* weights_arena, void* workspace);

/* Convolution units in reference registration order (I3D_doubled.py:229-334);
 * name is the state_dict prefix, e.g. "Mixed_3b.b1a" or "logits". */
int ivf_i3d_num_convs(const ivf_i3d_t* net);
int ivf_i3d_conv_info(const ivf_i3d_t* net, int i, char* name64, int* cout, int* cin, int* kT, int* kH,
                      int* kW, int* has_bn);
/* Pack one unit from reference-layout device tensors: w [Cout][Cin][kT][kH][kW];
 * BN tensors (NULL for the logits unit, which takes bias instead). */
int ivf_i3d_load_conv(ivf_i3d_t* net, int i, const float* w, const float* bn_gamma, const float* bn_beta,
                      const float* bn_mean, const float* bn_var, const float* bias, float bn_eps,
                      ivf_stream_t stream);

/* Model.forward, I3D_doubled.py:351-380, on b <= B clips.  x NCTHW.
 * logits/probs [b,K] outputs (either may be NULL); activations stay in the workspace. */
int ivf_i3d_forward(ivf_i3d_t* net, const float* x, int b, float* logits, float* probs,
                    ivf_stream_t stream);
/* Forward of an already perturbed channels-last clip held in the plan's input buffer. */
int ivf_i3d_forward_staged(ivf_i3d_t* net, int b, float* logits, float* probs, ivf_stream_t stream);
/* Device pointer of the plan's input buffer [B,T,H*W,4] (channels-last, C padded to 4). */
float* ivf_i3d_input_buffer(ivf_i3d_t* net);
/* Backward-data of the last forward: upstream dout [b,K] or one-hot target[b];
 * writes score[b] (optional), dx NCTHW (optional); the channels-last gradient of
 * the input stays in the workspace (ivf_i3d_input_grad_buffer). */
int ivf_i3d_backward(ivf_i3d_t* net, int b, const int* target, const float* dout, float* score,
                     float* dx, ivf_stream_t stream);
float* ivf_i3d_input_grad_buffer(ivf_i3d_t* net);

/* Named endpoint activations of the last forward (tests, Grad-CAM):
 * channels-last [b,T,H,W,ld]; returns IVF_ERR_BAD_ARG for an unknown name. */
int ivf_i3d_endpoint(const ivf_i3d_t* net, const char* name, float** ptr, int* T, int* H, int* W, int* C,
                     int* ld);
/* Bytes per stored element of those endpoints (and of every other activation / gradient buffer except the clip and
 * its gradient): 4 (float), or 2 (bf16) in an IVF_MATH_BF16ACT plan -- *ptr then addresses bf16 elements. */
int ivf_i3d_act_elem_bytes(const ivf_i3d_t* net);

/* The hot loop, smth:193-214, for b clips with per-clip masks, entirely on the
 * device: N iterations of sigmoid/L1/TV -> freeze -> forward -> score -> backward
 * -> freeze backward -> Adam.  raw_mask, exp_avg, exp_avg_sq [b,T] in/out;
 * target [b]; traj [N,b,4] = (loss,l1,tv,score) or NULL; first_step = Adam step
 * number of the first iteration (1 for a fresh search); mode = the perturbation the loop
 * optimises through (temporalMaskType, smth:121,202): 0 freeze, 1 reverse. */
int ivf_i3d_search(ivf_i3d_t* net, const float* x, int b, const int* target, float* raw_mask,
                   float* exp_avg, float* exp_avg_sq, float lam1, float lam2, float lr, float beta1,
                   float beta2, float eps, int N, int first_step, int mode, float* traj,
                   ivf_stream_t stream);

/* Scores of perturbed clips (init_mask, mask.py:121-154, and the reverse score,
 * smth:234-235): mode 0 = freeze with mask [b,T] as given (no sigmoid), mode 1 =
 * reverse with mask [b,T]; probs [b,K]. */
int ivf_i3d_perturbed_forward(ivf_i3d_t* net, const float* x, int b, const float* mask, int mode,
                              float* probs, ivf_stream_t stream);

/* Spatio-temporal mask search (extension, see ivf_stmask_*): N iterations on raw [b,T,gh,gw] with per-pixel freeze
 * through this plan; A_H [H,gh], A_W [W,gw] from ivf_stmask_axis_weights, on the device; traj [N,b,5] (optional) =
 * (J, l1, tvt, tvs, score); ws = ivf_stsearch_workspace_bytes(b, T, H, W, gh, gw) bytes from the caller, 256-byte
 * aligned.  One stream, no host synchronisation, no allocation.  _stperturbed_forward: the network on x frozen per
 * pixel by M [b,T,H*W]. */
int ivf_i3d_stsearch(ivf_i3d_t* net, const float* x, int b, const int* target, float* raw, float* exp_avg,
                     float* exp_avg_sq, const float* A_H, const float* A_W, int gh, int gw, float lam1, float lam2,
                     float lam3, float lr, float beta1, float beta2, float eps, int N, int first_step, float* traj,
                     void* ws, ivf_stream_t stream);
int ivf_i3d_stperturbed_forward(ivf_i3d_t* net, const float* x, int b, const float* M, float* probs,
                                ivf_stream_t stream);

/* Scores of every one-blob candidate of b clips (see ivf_blob_count): scores [b,n] = probs[target[clip]] of the
 * perturbed clip under mode (0 freeze, 1 reverse).  Runs the grid in chunks of the plan's B rows (stage -> forward ->
 * pick), chunks crossing clip boundaries; one stream, no host sync, no allocation. */
int ivf_i3d_blob_scores(ivf_i3d_t* net, const float* x, int b, const int* target, int max_len, int mode,
                        float* scores, ivf_stream_t stream);
/* Scores of every one-box candidate of b clips (see ivf_box_count): scores [b,n] = probs[target[clip]] of the clip
 * frozen per pixel by the candidate's expanded mask, in chunks of the plan's B rows (ivf_box_stage -> forward); b may
 * exceed B.  One stream, no host synchronisation, no allocation. */
int ivf_i3d_box_scores(ivf_i3d_t* net, const float* x, int b, const int* target, const float* A_H, const float* A_W, int gh,
                      int gw, int max_len, int mh, int mw, float* scores, ivf_stream_t stream);
/* Scores of the n RISE masks of b clips (extension, see ivf_rise_*): scores [b,n] = probs[target[clip]] of the clip
 * frozen per pixel by mask k, in chunks of the plan's B rows (ivf_rise_stage -> forward -> pick); b may exceed B.  One
 * stream, no host synchronisation, no allocation, no scratch beyond scores. */
int ivf_i3d_rise_scores(ivf_i3d_t* net, const float* x, int b, const int* target, const float* A_H, const float* A_W,
                        int gt, int gh, int gw, int n, unsigned seed, unsigned thresh, float* scores,
                        ivf_stream_t stream);
/* Scores of the n (P+1) Shapley rows of each of b clips (extension, see ivf_shap_*): scores [b,n,P+1] =
 * probs[target[clip]] of the clip frozen per pixel by prefix j of permutation k (ranks [n,P] on the device), in chunks
 * of the plan's B rows (ivf_shap_stage -> forward -> pick); b may exceed B.  One stream, no host synchronisation, no
 * allocation, no scratch beyond scores. */
int ivf_i3d_shap_scores(ivf_i3d_t* net, const float* x, int b, const int* target, const float* A_H, const float* A_W,
                        int gt, int gh, int gw, int n, const unsigned short* ranks, float* scores, ivf_stream_t stream);
/* Scores of the n+1 linear-surrogate rows of each of b clips (extension, see ivf_lin_*): scores [b,n+1] =
 * probs[target[clip]] of the clip frozen per pixel by sample row k of bits [n, ceil(P/32)] (on the device), entry n the
 * fully frozen clip, in chunks of the plan's B rows (ivf_lin_stage -> forward -> pick); b may exceed B.  One stream, no
 * host synchronisation, no allocation, no scratch beyond scores. */
int ivf_i3d_lin_scores(ivf_i3d_t* net, const float* x, int b, const int* target, const float* A_H, const float* A_W,
                       int gt, int gh, int gw, int n, const unsigned* bits, float* scores, ivf_stream_t stream);
/* Scores of the deletion / insertion rows of each of b clips (extension, see ivf_curve_*): scores [b,ncurves,J+1] =
 * probs[target[clip]] of the clip frozen per pixel by row j of each curve under the clip's own table ranks [b,P], in
 * chunks of the plan's B rows across clip and curve boundaries (ivf_curve_stage -> forward -> pick); b may exceed B.
 * One stream, no host synchronisation, no allocation, no scratch beyond scores. */
int ivf_i3d_curve_scores(ivf_i3d_t* net, const float* x, int b, const int* target, const float* A_H, const float* A_W,
                         int gt, int gh, int gw, const unsigned short* ranks, int curves, int step, float* scores,
                         ivf_stream_t stream);
/* Scores of the nc + 1 Score-CAM rows of each of b clips (extension, see ivf_scorecam_*): scores [b,nc+1] =
 * probs[target[clip]] of the clip perturbed by the expanded plane of channel k of F [b,nc,gt,gh,gw], the last the
 * baseline row, in chunks of the plan's B rows across clip boundaries (ivf_scorecam_stage -> forward -> pick); b may
 * exceed B.  One stream, no host synchronisation, no allocation, no scratch beyond scores. */
int ivf_i3d_scorecam_scores(ivf_i3d_t* net, const float* x, int b, const int* target, const float* A_H, const float* A_W,
                            int gt, int gh, int gw, const float* F, int nc, int perturb, float* scores,
                            ivf_stream_t stream);

/* Integrated Gradients of b clips through this plan (extension, see ivf_ig_*): the b*K path points run in chunks of the
 * plan's B rows across clip boundaries (ivf_ig_stage -> forward -> backward -> ivf_ig_accumulate), then ivf_ig_finish;
 * b may exceed B.  The score is what ivf_i3d_backward differentiates (target [b]).  ig_map [b,T,HW], frames and
 * abs_frames [b,T], total [b]; path_scores [b,K] (optional): the score at every path point; ws =
 * ivf_ig_workspace_bytes(b, C, T, H*W, K) bytes from the caller, 256-byte aligned.  One stream, no host
 * synchronisation, no allocation.  _ig_path_scores: forward only (stage -> forward -> pick), scores [b,K]; with
 * alpha = {0} it scores the baseline itself. */
int ivf_i3d_ig(ivf_i3d_t* net, const float* x, int b, const int* target, int base_kind, const float* base,
               float base_value, const float* alpha, const float* w, int K, float* ig_map, float* frames,
               float* abs_frames, float* total, float* path_scores, void* ws, ivf_stream_t stream);
int ivf_i3d_ig_path_scores(ivf_i3d_t* net, const float* x, int b, const int* target, int base_kind, const float* base,
                           float base_value, const float* alpha, int K, float* scores, ivf_stream_t stream);

/* SmoothGrad, SmoothGrad^2 and VarGrad of b clips through this plan (extension, see ivf_sg_*): ivf_sg_range, then the
 * b*n (clip, sample) rows in chunks of the plan's B rows across clip boundaries (ivf_sg_stage -> forward -> backward ->
 * ivf_sg_accumulate), then ivf_sg_finish; b may exceed B.  The score is what ivf_i3d_backward differentiates (target
 * [b]).  sg_map, sq_map, var_map [b,T,HW]; sg_frames, sq_frames, var_frames [b,T]; sample_scores [b,n] and sigma [b]
 * (both optional): the score of every sample and the noise scale of every clip; ws = ivf_sg_workspace_bytes(b, C, T,
 * H*W, n) bytes from the caller, 256-byte aligned.  n = 1, level = 0 is the plain gradient map sum_c |d score / d x|.
 * One stream, no host synchronisation, no allocation. */
int ivf_i3d_smoothgrad(ivf_i3d_t* net, const float* x, int b, const int* target, int n, float level, unsigned seed,
                       float* sg_map, float* sq_map, float* var_map, float* sg_frames, float* sq_frames,
                       float* var_frames, float* sample_scores, float* sigma, void* ws, ivf_stream_t stream);

/* GradCamVideo.__call__ for archType "I3D" / target layer Mixed_5c,
 * grad_cam_videos.py:64-142, for b clips.  target[b] (device) selects the class;
 * cam [b,T'*(T/T'),out_h,out_w] (input_spatial_size, grad_cam_videos.py:54-57);
 * probs [b,K] optional. */
int ivf_i3d_gradcam(ivf_i3d_t* net, const float* x, int b, const int* target, int per_frame, int out_h,
                    int out_w, float* cam, float* probs, ivf_stream_t stream);
/* The same for any single endpoint of the model as target layer (pytorch-grad-cam/grad-cam.py:23-54
 * hooks the OUTPUT of the named module: Conv3d_1a_7x7, MaxPool3d_2a_3x3, ..., Mixed_5c): forward,
 * backward-data from the class score down to that endpoint with ITS gradient left ungated, then the
 * Grad-CAM reduction on [T',H',W',C'] and the resize with step = T / T'. */
int ivf_i3d_gradcam_layer(ivf_i3d_t* net, const float* x, int b, const int* target, const char* layer,
                          int per_frame, int out_h, int out_w, float* cam, float* probs, ivf_stream_t stream);
/* The Grad-CAM family on one endpoint (a documented extension): ONE forward and ONE backward down to `layer` as in
 * ivf_i3d_gradcam_layer, then ivf_cam_reduce for the n_kinds kinds of kinds_host and ivf_cam_resize_normalise per
 * kind.  cam [n_kinds,b,T'*(T/T'),out_h,out_w].  The scratch is part of the plan's workspace. */
int ivf_i3d_cam_layer(ivf_i3d_t* net, const float* x, int b, const int* target, const char* layer, int n_kinds,
                      const int* kinds_host, int per_frame, int out_h, int out_w, float* cam, float* probs,
                      ivf_stream_t stream);
/* The same up to the reduction: cam [n_kinds,b,T',H',W'] un-resized, weights [n_kinds,b,C], fp32 copies of the
 * activations and gradients the reduction read, [b,T',H',W',C], and probs [b,K]; every output optional. */
int ivf_i3d_cam_raw(ivf_i3d_t* net, const float* x, int b, const int* target, const char* layer, int n_kinds,
                    const int* kinds_host, float* cam, float* weights, float* feat, float* grad, float* probs,
                    ivf_stream_t stream);
/* argmax over K of probs [b,K] -> target [b] (np.argmax, grad_cam_videos.py:69-70). */
int ivf_argmax(const float* probs, int b, int K, int* target, ivf_stream_t stream);

/* ------------------------------------------------------------------ CLSTM_4 */

typedef struct {
  int B;                 /* maximum clips per call */
  int C, T, H, W;        /* clip geometry, reference NCTHW (KTH: C in {1,3}, 32, 120, 160) */
  int hidden;            /* nb_lstm_units (<= 4) */
  int layers;            /* lstm_layers */
  int kernel;            /* conv_kernel_size[0], odd */
  int stride;            /* conv_stride of the input convolutions */
  int num_classes;
  int softmax;           /* add_softmax (CLSTM_4.py:82-83) */
  int batch_norm;        /* the single shared BatchNorm2d (convolution_lstm.py:85,123) */
  int out_step;          /* step whose pooled top-layer output feeds endFC: the LAST effective
                            step (CLSTM_4.py:78-80 with use_entire_seq=False) */
  /* use_entire_seq=True (CLSTM_4.py:73-76): endFC reads the pooled top-layer outputs of ALL the
   * effective steps reached, concatenated per clip in step order (n_out_steps * feat inputs);
   * n_out_steps == 0 selects the single out_step above. */
  int n_out_steps;
  int out_steps[16];
} ivf_clstm_config;

typedef struct ivf_clstm ivf_clstm_t;

/* models/CLSTM_4.Model + models/convolution_lstm.ConvLSTM (forward :96-132, cell :38-48). */
int ivf_clstm_create(const ivf_clstm_config* cfg, ivf_clstm_t** out);
void ivf_clstm_destroy(ivf_clstm_t* net);
size_t ivf_clstm_weights_bytes(const ivf_clstm_t* net);
size_t ivf_clstm_workspace_bytes(const ivf_clstm_t* net);
int ivf_clstm_bind(ivf_clstm_t* net, void* weights_arena, void* workspace);
/* One cell's reference tensors: Wx* [hid][cin][k][k] + bias [hid], Wh* [hid][hid][k][k];
 * gate order i, f, c, o (convolution_lstm.py:22-29). */
int ivf_clstm_load_cell(ivf_clstm_t* net, int layer, const float* wxi, const float* wxf, const float* wxc,
                        const float* wxo, const float* bxi, const float* bxf, const float* bxc,
                        const float* bxo, const float* whi, const float* whf, const float* whc,
                        const float* who, ivf_stream_t stream);
/* clstm.bn.* (NULL when batch_norm == 0) and endFC.{weight [K][feat], bias}. */
int ivf_clstm_load_head(ivf_clstm_t* net, const float* bn_gamma, const float* bn_beta, const float* bn_mean,
                        const float* bn_var, const float* fc_w, const float* fc_b, float bn_eps,
                        ivf_stream_t stream);
/* Model.forward, CLSTM_4.py:69-85, on b <= B clips (x NCTHW). */
int ivf_clstm_forward(ivf_clstm_t* net, const float* x, int b, float* logits, float* probs,
                      ivf_stream_t stream);
/* BPTT backward-data of the last forward: dx NCTHW [b,C,T,H,W]. */
int ivf_clstm_backward(ivf_clstm_t* net, int b, const int* target, const float* dout, float* score, float* dx,
                       ivf_stream_t stream);
/* The hot loop (KTH:250-270) with the ConvLSTM backbone; arguments as ivf_i3d_search. */
int ivf_clstm_search(ivf_clstm_t* net, const float* x, int b, const int* target, float* raw_mask,
                     float* exp_avg, float* exp_avg_sq, float lam1, float lam2, float lr, float beta1,
                     float beta2, float eps, int N, int first_step, int mode, float* traj,
                     ivf_stream_t stream);
int ivf_clstm_perturbed_forward(ivf_clstm_t* net, const float* x, int b, const float* mask, int mode,
                                float* probs, ivf_stream_t stream);

/* Spatio-temporal mask search (extension, see ivf_stmask_*): N iterations on raw [b,T,gh,gw] with per-pixel freeze
 * through this plan; A_H [H,gh], A_W [W,gw] from ivf_stmask_axis_weights, on the device; traj [N,b,5] (optional) =
 * (J, l1, tvt, tvs, score); ws = ivf_stsearch_workspace_bytes(b, T, H, W, gh, gw) bytes from the caller, 256-byte
 * aligned.  One stream, no host synchronisation, no allocation.  _stperturbed_forward: the network on x frozen per
 * pixel by M [b,T,H*W]. */
int ivf_clstm_stsearch(ivf_clstm_t* net, const float* x, int b, const int* target, float* raw, float* exp_avg,
                     float* exp_avg_sq, const float* A_H, const float* A_W, int gh, int gw, float lam1, float lam2,
                     float lam3, float lr, float beta1, float beta2, float eps, int N, int first_step, float* traj,
                     void* ws, ivf_stream_t stream);
int ivf_clstm_stperturbed_forward(ivf_clstm_t* net, const float* x, int b, const float* M, float* probs,
                                ivf_stream_t stream);

/* ivf_i3d_blob_scores with the ConvLSTM backbone (candidates staged NCTHW). */
int ivf_clstm_blob_scores(ivf_clstm_t* net, const float* x, int b, const int* target, int max_len, int mode,
                          float* scores, ivf_stream_t stream);
/* Scores of every one-box candidate of b clips (see ivf_box_count): scores [b,n] = probs[target[clip]] of the clip
 * frozen per pixel by the candidate's expanded mask, in chunks of the plan's B rows (ivf_box_stage -> forward); b may
 * exceed B.  One stream, no host synchronisation, no allocation. */
int ivf_clstm_box_scores(ivf_clstm_t* net, const float* x, int b, const int* target, const float* A_H, const float* A_W, int gh,
                      int gw, int max_len, int mh, int mw, float* scores, ivf_stream_t stream);
/* ivf_i3d_rise_scores with the ConvLSTM backbone (rows staged NCTHW). */
int ivf_clstm_rise_scores(ivf_clstm_t* net, const float* x, int b, const int* target, const float* A_H, const float* A_W,
                          int gt, int gh, int gw, int n, unsigned seed, unsigned thresh, float* scores,
                          ivf_stream_t stream);
/* ivf_i3d_shap_scores with the ConvLSTM backbone (rows staged NCTHW). */
int ivf_clstm_shap_scores(ivf_clstm_t* net, const float* x, int b, const int* target, const float* A_H, const float* A_W,
                          int gt, int gh, int gw, int n, const unsigned short* ranks, float* scores, ivf_stream_t stream);
/* ivf_i3d_lin_scores with the ConvLSTM backbone (rows staged NCTHW). */
int ivf_clstm_lin_scores(ivf_clstm_t* net, const float* x, int b, const int* target, const float* A_H, const float* A_W,
                         int gt, int gh, int gw, int n, const unsigned* bits, float* scores, ivf_stream_t stream);
/* ivf_i3d_curve_scores with the ConvLSTM backbone (rows staged NCTHW). */
int ivf_clstm_curve_scores(ivf_clstm_t* net, const float* x, int b, const int* target, const float* A_H, const float* A_W,
                           int gt, int gh, int gw, const unsigned short* ranks, int curves, int step, float* scores,
                           ivf_stream_t stream);
/* ivf_i3d_scorecam_scores with the ConvLSTM backbone (rows staged NCTHW). */
int ivf_clstm_scorecam_scores(ivf_clstm_t* net, const float* x, int b, const int* target, const float* A_H,
                              const float* A_W, int gt, int gh, int gw, const float* F, int nc, int perturb,
                              float* scores, ivf_stream_t stream);

/* Integrated Gradients of b clips through this plan (extension, see ivf_ig_*): the b*K path points run in chunks of the
 * plan's B rows across clip boundaries (ivf_ig_stage -> forward -> backward -> ivf_ig_accumulate), then ivf_ig_finish;
 * b may exceed B.  The score is what ivf_clstm_backward differentiates (target [b]).  ig_map [b,T,HW], frames and
 * abs_frames [b,T], total [b]; path_scores [b,K] (optional): the score at every path point; ws =
 * ivf_ig_workspace_bytes(b, C, T, H*W, K) bytes from the caller, 256-byte aligned.  One stream, no host
 * synchronisation, no allocation.  _ig_path_scores: forward only (stage -> forward -> pick), scores [b,K]; with
 * alpha = {0} it scores the baseline itself. */
int ivf_clstm_ig(ivf_clstm_t* net, const float* x, int b, const int* target, int base_kind, const float* base,
               float base_value, const float* alpha, const float* w, int K, float* ig_map, float* frames,
               float* abs_frames, float* total, float* path_scores, void* ws, ivf_stream_t stream);
int ivf_clstm_ig_path_scores(ivf_clstm_t* net, const float* x, int b, const int* target, int base_kind, const float* base,
                           float base_value, const float* alpha, int K, float* scores, ivf_stream_t stream);
/* ivf_i3d_smoothgrad with the ConvLSTM backbone (rows staged NCTHW; the score is what ivf_clstm_backward differentiates). */
int ivf_clstm_smoothgrad(ivf_clstm_t* net, const float* x, int b, const int* target, int n, float level, unsigned seed,
                         float* sg_map, float* sq_map, float* var_map, float* sg_frames, float* sq_frames,
                         float* var_frames, float* sample_scores, float* sigma, void* ws, ivf_stream_t stream);

/* Grad-CAM on the ConvLSTM's pooled layer outputs, stored [B,T,hid,plane] (plane = Hp*Wp), fp32:
 * weights[b,c] = mean over (selected steps, plane) of grad (grad_cam_videos.py:98), cam[b,e,:] =
 * relu(sum_c weights[b,c] * feat[b,step_e,c,:]) (:101-110), cam [B,n_steps,plane].  steps_host: n_steps (<= 64)
 * HOST ints inside [0,T), NULL = 0 .. n_steps-1; they travel as a kernel argument.  One workgroup per
 * (channel, clip), no atomics: a clip's result does not depend on B. */
int ivf_clstm_gradcam_reduce(const float* feat, const float* grad, const int* steps_host, int n_steps,
                             float* weights, float* cam, int B, int T, int hid, int plane, ivf_stream_t stream);
/* The effective steps that lie inside the clip (convolution_lstm.py:129-130), increasing HOST ints: the map stack
 * of Grad-CAM target 'clstm'.  Default: the plan's output steps. */
int ivf_clstm_set_cam_steps(ivf_clstm_t* net, const int* steps_host, int n_steps);
/* GradCamVideo.__call__ for archType "CLSTM" (grad_cam_videos.py:64-142 over pytorch-grad-cam/grad-cam.py:33-49)
 * on b clips: forward, backward truncated above the target, reduction, resize + normalise.
 * layer -1 is the reference's branch: the top layer's pooled outputs at the effective steps (n maps, each
 * repeated T / n times; cam [b, n*(T/n), out_h, out_w]) with the gradient endFC sends into them.
 * layer 0 .. layers-1 is an EXTENSION: that layer's pooled output at every step with the gradient of the class
 * score through the layers above and their recurrences (cam [b,T,out_h,out_w]).
 * target [b] device ints, NULL = argmax of the output; probs [b,K] optional. */
int ivf_clstm_gradcam(ivf_clstm_t* net, const float* x, int b, const int* target, int layer, int per_frame,
                      int out_h, int out_w, float* cam, float* probs, ivf_stream_t stream);
/* The same up to the reduction: cam [b,n,Hp,Wp] un-resized, weights [b,hid], and copies of the features and
 * gradients the reduction read, [b,n,hid,Hp,Wp] (n as above); every output optional. */
int ivf_clstm_gradcam_raw(ivf_clstm_t* net, const float* x, int b, const int* target, int layer, float* cam,
                          float* weights, float* feat, float* grad, float* probs, ivf_stream_t stream);
/* The Grad-CAM family on the same [B,T,hid,plane] buffers and step list as ivf_clstm_gradcam_reduce:
 * positions = selected steps x plane; kinds, rows and rules as ivf_cam_reduce; weights [n_kinds,B,hid] (optional
 * unless kind 0 is asked for: its kernels keep the weights there), cam [n_kinds,B,n_steps,plane]; hid <=
 * IVF_CAM_MAX_HID.  One workgroup per clip, fixed summation order, no atomics.  The maps are post-BN and can be
 * negative: s_k may be negative or tiny and Grad-CAM++'s denominator may pass through 0; values propagate. */
int ivf_clstm_cam_reduce(const float* feat, const float* grad, const int* steps_host, int n_steps, int n_kinds,
                         const int* kinds_host, float* weights, float* cam, int B, int T, int hid, int plane,
                         ivf_stream_t stream);
/* ivf_clstm_gradcam / ivf_clstm_gradcam_raw for n_kinds kinds from one forward and one backward:
 * cam [n_kinds,b,n*(T/n),out_h,out_w]; raw: cam [n_kinds,b,n,Hp,Wp], weights [n_kinds,b,hid], feat and grad
 * [b,n,hid,Hp,Wp] as ivf_clstm_gradcam_raw. */
int ivf_clstm_cam(ivf_clstm_t* net, const float* x, int b, const int* target, int layer, int n_kinds,
                  const int* kinds_host, int per_frame, int out_h, int out_w, float* cam, float* probs,
                  ivf_stream_t stream);
int ivf_clstm_cam_raw(ivf_clstm_t* net, const float* x, int b, const int* target, int layer, int n_kinds,
                      const int* kinds_host, float* cam, float* weights, float* feat, float* grad, float* probs,
                      ivf_stream_t stream);
/* Workspace views of one layer after a forward / backward: pooled outputs X and their gradient dX, both
 * [b,T,hid,Hp,Wp]; every output optional. */
int ivf_clstm_layer_buffers(ivf_clstm_t* net, int layer, const float** X, const float** dX, int* hid, int* Hp,
                            int* Wp);

/* Per-layer kernel selection.  ivf_i3d_autotune times every candidate variant of every
 * convolution (forward and backward-data) on `b` clips and keeps the fastest; the result is
 * 2*ivf_i3d_num_conv_ops() ints that can be read and installed again, e.g. broadcast from
 * rank 0 so all GPUs of a sharded run use identical kernels (bit-identical per-clip results). */
int ivf_i3d_num_conv_ops(const ivf_i3d_t* net);
int ivf_i3d_autotune(ivf_i3d_t* net, int b, int reps, ivf_stream_t stream);
int ivf_i3d_get_tuning(const ivf_i3d_t* net, int* variants_host);
int ivf_i3d_set_tuning(ivf_i3d_t* net, const int* variants_host);

/* Algorithmic forward FLOPs of all Unit3D convolutions for one clip (2*MAC, real
 * channel counts; backward-data costs the same again).  SURVEY.md section 8d. */
double ivf_i3d_conv_flops_per_clip(const ivf_i3d_t* net);

/* ------------------------------------------------------------------ visualisation */

/* create_image_arrays, visualisation.py:96-130 (RESIZE_FLAG = 0 as in both drivers): per frame the strip
 * original | heat-map overlay | perturbed clip, BGR uint8 [T][H][3W][3].  clip, perturbed [3,T,H,W]
 * (RGB planes, 0..255), cam [T,H,W] in [0,1] (GradCamVideo output), lut_bgr [256][3] =
 * cv2.COLORMAP_JET in BGR order (host-provided), frame_max: T floats of workspace.
 * overlay = (lut[uint8(255 cam)] + original) / max over the frame, then uint8(255 .). */
int ivf_viz_blend(const float* clip, const float* cam, const float* perturbed, const unsigned char* lut_bgr,
                  float* frame_max, unsigned char* out, int T, int H, int W, ivf_stream_t stream);
/* vizualize_results_on_gradcam, visualisation.py:35-64: the red (mask 1) / green (mask 0) dot row on the
 * third panel of every frame, 255 for the frame's own dot, 150 for the others; mask_snapped [T] holds 0/1
 * (find_temp_mask_red_dots :67-93 snaps the caller's mask first).  image_width/height: the reference's
 * defaults are 224 whatever the frame size. */
int ivf_viz_dots(unsigned char* img, const float* mask_snapped, int T, int H, int W3, int image_width,
                 int image_height, ivf_stream_t stream);

/* ------------------------------------------------------------------ TF-style ConvLSTM search variant
 *
 * DOCUMENTED EXTENSION, PARITY UNPINNED: the reference's TensorFlow half (video_features_tf/mask/find_mask_kth.py:300-372,
 * 431-452; mask/gradcam.py:28-111; models/clstm.py:9-52, 87-126) runs the temporal-mask search and a per-frame
 * Grad-CAM over a Keras ConvLSTM2D stack.  TF 1.12 / Keras cannot be installed where this library is built, so no
 * output of that code pins these entry points; they follow the published Keras ConvLSTM2D definition as the call site
 * configures it (csrc/tf_clstm.hip has the equations): x-part conv with `padding` 'valid' | 'same' (TensorFlow rule)
 * and `stride`, recurrent conv 'same' / stride 1, kernel kh x kw (any, e.g. the configs' 3 x 5), gate order i, f, c, o,
 * hard-sigmoid recurrent activation (TF 1.12 default), MaxPooling2D(2x2) per frame after every layer, no batch norm
 * (find_mask_kth.py:331), dense head over the flattened (NHWC) last element or whole sequence.
 * Weights in Keras layouts: kernel [kh][kw][Cin][4F], recurrent_kernel [kh][kw][F][4F], bias [4F], dense kernel
 * [inputs][classes].  Clips are NCTHW like everywhere else in this library. */
typedef struct {
  int B;                      /* maximum clips per call */
  int C, T, H, W;             /* clip geometry */
  int layers;                 /* ConvLSTM2D blocks (<= 8) */
  int units[8];               /* filters per block (FLAGS.layers) */
  int kh, kw;                 /* kernel_size_1, kernel_size_2 */
  int stride;                 /* FLAGS.strides */
  int padding;                /* 0 'valid', 1 'same' */
  int recurrent_hard_sigmoid; /* 1: hard_sigmoid (TF 1.12 Keras default), 0: sigmoid */
  int only_last;              /* only_last_element_for_fc == 'yes' */
  int num_classes;
} ivf_tfclstm_config;

typedef struct ivf_tfclstm ivf_tfclstm_t;

int ivf_tfclstm_create(const ivf_tfclstm_config* cfg, ivf_tfclstm_t** out);
void ivf_tfclstm_destroy(ivf_tfclstm_t* net);
size_t ivf_tfclstm_weights_bytes(const ivf_tfclstm_t* net);
size_t ivf_tfclstm_workspace_bytes(const ivf_tfclstm_t* net);
int ivf_tfclstm_bind(ivf_tfclstm_t* net, void* weights_arena, void* workspace);
/* conv output (Ho, Wo), pooled (Hp, Wp) and filters of a block; inputs of the dense head */
int ivf_tfclstm_layer_dims(const ivf_tfclstm_t* net, int layer, int* Ho, int* Wo, int* Hp, int* Wp, int* units);
int ivf_tfclstm_fc_inputs(const ivf_tfclstm_t* net);
/* Workspace views of one block after a forward / backward (test support): its output sequence H [b,T,F,Ho,Wo], its
 * pooled output X [b,T,F,Hp,Wp] and the gradient dX that arrives at X (same shape); every output optional,
 * dimensions from ivf_tfclstm_layer_dims. */
int ivf_tfclstm_layer_buffers(ivf_tfclstm_t* net, int layer, const float** H, const float** X, const float** dX);
int ivf_tfclstm_load_layer(ivf_tfclstm_t* net, int layer, const float* kernel, const float* recurrent_kernel,
                           const float* bias, ivf_stream_t stream);
int ivf_tfclstm_load_head(ivf_tfclstm_t* net, const float* dense_kernel, const float* dense_bias, ivf_stream_t stream);
/* clstm.clstm(x) + softmax (find_mask_kth.py:331-332): logits / probs [b,K] (either may be NULL) */
int ivf_tfclstm_forward(ivf_tfclstm_t* net, const float* x, int b, float* logits, float* probs, ivf_stream_t stream);
/* BPTT of probs[b, target[b]] to the clip: score [b] optional, dx NCTHW */
int ivf_tfclstm_backward(ivf_tfclstm_t* net, int b, const int* target, float* score, float* dx, ivf_stream_t stream);
/* the tf.scan freeze recurrence (find_mask_kth.py:318-327) with mask [b,T] AS GIVEN, then the model: probs [b,K].
 * (The TF graph always applies sigmoid to its mask variable, also in init_mask and in the baseline prediction: callers
 * that mimic it pass sigmoid(values).) */
int ivf_tfclstm_perturbed_forward(ivf_tfclstm_t* net, const float* x, int b, const float* mask, float* probs,
                                  ivf_stream_t stream);
/* N iterations of the search (find_mask_kth.py:356-372, 431-452) on the device; tf.train.AdamOptimizer's update
 * (epsilon beside sqrt(v) before the bias correction); traj [N,b,4] = (loss, l1, tv, score) or NULL */
int ivf_tfclstm_search(ivf_tfclstm_t* net, const float* x, int b, const int* target, float* raw_mask, float* exp_avg,
                       float* exp_avg_sq, float lam1, float lam2, float lr, float beta1, float beta2, float eps, int N,
                       int first_step, float* traj, ivf_stream_t stream);
/* mask/gradcam.py:28-111: per-frame Grad-CAM on the last ConvLSTM2D's output sequence from the class LOGIT;
 * mask [b,T] as given to the freeze recurrence (NULL: unperturbed clip); per_frame 1 = normalization_mode 'frame',
 * 0 = 'sequence'; cam [b,T,out_h,out_w] (bilinear resize restating skimage.transform.resize, unpinned) */
int ivf_tfclstm_gradcam(ivf_tfclstm_t* net, const float* x, int b, const float* mask, const int* target, int per_frame,
                        int out_h, int out_w, float* cam, float* probs, ivf_stream_t stream);

/* ------------------------------------------------------------------ measurement */

/* HIP-event timing of the convolution launches on their own stream, sampled on every
 * `every`-th iteration of ivf_*_search (bench.py's roofline leg; every = 0: on every launch, also
 * of a direct ivf_conv3d call, which the tests of the dispatch use).  collect: arrays of
 * IVF_PROFILE_CLASSES entries indexed by kernel variant id (IVF_CONV_IGEMM_BASE + tile for
 * fp32, +3 for split-bf16; IVF_CONV_HALO_BASE + i): summed kernel milliseconds, launch count
 * and algorithmic FLOPs of the sampled launches. */
#define IVF_PROFILE_CLASSES 96
int ivf_profile_enable(int every, int max_launches);
int ivf_profile_disable(void);
int ivf_profile_collect(double* kernel_ms_host, long long* launches_host, double* flops_host);
/* The same sample per launch SITE of an I3D plan (site = 2 * op index + direction; names from
 * ivf_i3d_site_name, count from ivf_i3d_num_sites): summed milliseconds, launches, algorithmic FLOPs and the
 * kernel variant that served the site.  Does not reset the sample: call it before ivf_profile_collect. */
int ivf_profile_collect_sites(double* kernel_ms_host, long long* launches_host, double* flops_host,
                              int* variant_host, int max_sites);
int ivf_i3d_num_sites(const ivf_i3d_t* net);
int ivf_i3d_site_name(const ivf_i3d_t* net, int site, char* name64);
/* Kernel template instance behind a class id ("" until that class has been launched). */
const char* ivf_profile_class_name(int cls);

#ifdef __cplusplus
}
#endif
#endif /* IVF_HIP_H */
