// Host sequencing shared by the three backbones (I3D, CLSTM_4, the TF ConvLSTM2D classifier): the mask search loop,
// the perturb-and-forward step and the chunk loop of the one-blob search.  Internal: not part of include/ivf_hip.h.
// A backbone provides a Backbone view of its plan (below); the extern "C" entries check their arguments and call in.
#pragma once
#include <algorithm>

#include "ivf_common.h"

namespace ivf {

// Per-plan scratch of the search loop: byte offsets into the plan's workspace.
struct SearchScratch {
  size_t score = 0, sig = 0, terms = 0, dreg = 0, dsig = 0, fbwd = 0;
  size_t partner = 0, weight = 0;   // 'reverse' pairing rows, int [B,T] and float [B,T] (plans with a reverse mode)

  // `take(bytes)` is the plan's workspace allocator; the order and the sizes are part of every plan's layout.
  template <class Take>
  void carve(Take&& take, size_t B, size_t T) {
    score = take(B * 4);
    sig = take(B * T * 4);
    terms = take(B * 2 * 4);
    dreg = take(B * T * 4);
    dsig = take(B * T * 4);
    fbwd = take(ivf_freeze_bwd_workspace_bytes((int)B, (int)T));
  }
  // The pairing kernels need B*T*8 bytes (partner + weight).  The ConvLSTM plan takes exactly that; the I3D plan has
  // always taken B*T*12, which is kept so that its workspace size does not move; the TF plan has no reverse mode.
  template <class Take>
  void carve_pairs(Take&& take, size_t B, size_t T, size_t bytes_per_frame) {
    partner = take(B * T * bytes_per_frame);
    weight = partner + B * T * sizeof(int);
  }
};

// What the shared code needs from a plan.  `forward` runs the network on the b rows staged in `in` (probs_out
// optional; the plan's own `probs` buffer is always written); `backward` is backward-data of that forward for
// target[b] into `din`, writing score[b].
struct Backbone {
  void* plan;
  int B, C, T, HW, K;         // plan batch, clip geometry, classes
  int layout;                 // of in / din, as the mask kernels name it: 0 NCTHW, 4 16-byte channels-last pixels
  float *in, *din;            // staged input and its gradient
  const float* probs;         // [B,K] of the last forward
  char* ws;
  const SearchScratch* sc;
  int (*forward)(void* plan, int b, float* probs_out, hipStream_t s);
  int (*backward)(void* plan, int b, const int* target, float* score, hipStream_t s);

  template <class U>
  U* at(size_t off) const { return (U*)(ws + off); }
};

// x perturbed by `mask` [b,T] (values in [0,1]) into the staged input: mode 0 freeze, 1 reverse (mask.py:38-57)
static inline int stage_perturbed(const Backbone& v, const float* x, const float* mask, int b, int mode, hipStream_t s) {
  if (mode == 0) return ivf_freeze_fwd(x, mask, v.in, b, v.C, v.T, v.HW, 1, v.layout, s);
  int* partner = v.at<int>(v.sc->partner);
  float* weight = v.at<float>(v.sc->weight);
  IVF_PROPAGATE(ivf_submask_pairs_batched(mask, b, v.T, 0.1f, partner, weight, s));
  return ivf_reverse_fwd_batched(x, partner, weight, v.in, b, v.C, v.T, v.HW, v.layout, s);
}

static inline int run_perturbed_forward(const Backbone& v, const float* x, const float* mask, int b, int mode,
                                        float* probs, hipStream_t s) {
  IVF_PROPAGATE(stage_perturbed(v, x, mask, b, mode, s));
  return v.forward(v.plan, b, probs, s);
}

// N iterations of the hot loop (FindMasksComparison_I3D_smth.py:193-214): sigmoid + L1 + TV, perturb, network forward
// and backward, perturbation backward, Adam.  eps_at(step) is the Adam epsilon of step `step` (torch: eps itself;
// tf.train.Adam: see ivf_tfclstm_search).  prof_set_iteration only gates the launch profiler of the conv3d launchers,
// which the I3D plan alone reaches, so it is called for every backbone.
template <class EpsAt>
static int run_search(const Backbone& v, const float* x, int b, const int* target, float* raw_mask, float* exp_avg,
                      float* exp_avg_sq, float lam1, float lam2, float lr, float beta1, float beta2, EpsAt eps_at,
                      int N, int first_step, int mode, float* traj, hipStream_t s) {
  const SearchScratch& c = *v.sc;
  float *sig = v.at<float>(c.sig), *terms = v.at<float>(c.terms), *dreg = v.at<float>(c.dreg);
  float *dsig = v.at<float>(c.dsig), *score = v.at<float>(c.score);
  for (int it = 0; it < N; ++it) {
    prof_set_iteration(it);
    IVF_PROPAGATE(ivf_mask_reg(raw_mask, b, v.T, lam1, lam2, sig, terms, dreg, s));            // smth:198-200
    IVF_PROPAGATE(stage_perturbed(v, x, sig, b, mode, s));                                      // smth:202
    IVF_PROPAGATE(v.forward(v.plan, b, nullptr, s));                                            // smth:202-205
    IVF_PROPAGATE(v.backward(v.plan, b, target, score, s));                                     // smth:213
    if (mode == 0)
      IVF_PROPAGATE(ivf_freeze_bwd(x, sig, v.din, dsig, nullptr, b, v.C, v.T, v.HW, 1, v.layout, v.at<void>(c.fbwd), s));
    else
      IVF_PROPAGATE(ivf_reverse_bwd(x, v.at<int>(c.partner), v.din, dsig, b, v.C, v.T, v.HW, v.layout,
                                    v.at<void>(c.fbwd), s));
    const int step = first_step + it;
    IVF_PROPAGATE(ivf_search_step(raw_mask, sig, dsig, dreg, terms, score, exp_avg, exp_avg_sq,
                                  traj ? traj + (size_t)it * b * 4 : nullptr, b, v.T, step, lr, beta1, beta2,
                                  eps_at(step), s));                                            // smth:207-214
  }
  prof_set_iteration(-1);   // sampling off outside the loop
  return IVF_OK;
}

// Caller-owned scratch (StScratch, IgScratch below): byte offsets handed out in call order, each piece rounded up to
// 256 bytes; `top` is the total.  The order and the sizes of the calls are part of the ABI (ivf_*_workspace_bytes).
struct Bump256 {
  size_t top = 0;
  size_t take(size_t bytes) {
    size_t off = top;
    top += align_up(bytes, 256);
    return off;
  }
};

// The `total` rows of a flattened candidate list in chunks of the plan's B rows (chunks cross clip boundaries, so one
// clip still fills the plan): body(first, cnt) per chunk, the first non-OK code ends the loop.
template <class Body>
static inline int for_each_chunk(const Backbone& v, long long total, Body&& body) {
  for (long long first = 0; first < total; first += v.B)
    IVF_PROPAGATE(body(first, (int)std::min<long long>(v.B, total - first)));
  return IVF_OK;
}

// ---------------------------------------------------------------- spatio-temporal masks (maskType 'spacetime')
// An extension without a counterpart in the reference (stmask_ops.hip).  Its scratch belongs to the CALLER
// (ivf_stsearch_workspace_bytes), so no plan's workspace size or carve order moves.
struct StScratch {
  size_t M = 0, dM = 0, sig = 0, dreg = 0, dsig = 0, terms = 0, score = 0;

  // byte offsets of the pieces, each 256-byte aligned; returns the total
  size_t carve(size_t B, size_t T, size_t HW, size_t cells) {
    Bump256 a;
    M = a.take(B * T * HW * 4);
    dM = a.take(B * T * HW * 4);
    sig = a.take(B * T * cells * 4);
    dreg = a.take(B * T * cells * 4);
    dsig = a.take(B * T * cells * 4);
    terms = a.take(B * 3 * 4);
    score = a.take(B * 4);
    return a.top;
  }
};

// x frozen per pixel by M [b,T,HW] (values in [0,1]) into the staged input, then the network
static inline int run_st_perturbed_forward(const Backbone& v, const float* x, const float* M, int b, float* probs,
                                           hipStream_t s) {
  IVF_PROPAGATE(ivf_stfreeze_fwd(x, M, v.in, b, v.C, v.T, v.HW, v.layout, s));
  return v.forward(v.plan, b, probs, s);
}

// N iterations of the spacetime loop on raw [b,T,gh,gw]: sigmoid + regulariser, expand to M, per-pixel freeze, network
// forward and backward, dM, its adjoint expand, Adam.  traj rows [N,b,5] = (J, l1, tvt, tvs, score).  `ws`: the
// caller's ivf_stsearch_workspace_bytes(b, T, H, W, gh, gw) bytes.  As run_search: one stream, no host
// synchronisation, no allocation.
static int run_st_search(const Backbone& v, const float* x, int b, const int* target, float* raw, float* exp_avg,
                         float* exp_avg_sq, const float* A_H, const float* A_W, int gh, int gw, int H, int W, float lam1,
                         float lam2, float lam3, float lr, float beta1, float beta2, float eps, int N, int first_step,
                         float* traj, void* ws, hipStream_t s) {
  StScratch c;
  c.carve((size_t)b, (size_t)v.T, (size_t)v.HW, (size_t)gh * gw);
  char* w = (char*)ws;
  float *M = (float*)(w + c.M), *dM = (float*)(w + c.dM), *sig = (float*)(w + c.sig), *dreg = (float*)(w + c.dreg);
  float *dsig = (float*)(w + c.dsig), *terms = (float*)(w + c.terms), *score = (float*)(w + c.score);
  for (int it = 0; it < N; ++it) {
    prof_set_iteration(it);
    IVF_PROPAGATE(ivf_stmask_reg(raw, b, v.T, gh, gw, lam1, lam2, lam3, sig, terms, dreg, s));
    IVF_PROPAGATE(ivf_stmask_expand_fwd(sig, A_H, A_W, M, b, v.T, gh, gw, H, W, s));
    IVF_PROPAGATE(ivf_stfreeze_fwd(x, M, v.in, b, v.C, v.T, v.HW, v.layout, s));
    IVF_PROPAGATE(v.forward(v.plan, b, nullptr, s));
    IVF_PROPAGATE(v.backward(v.plan, b, target, score, s));
    IVF_PROPAGATE(ivf_stfreeze_bwd(x, M, v.din, dM, b, v.C, v.T, v.HW, v.layout, s));
    IVF_PROPAGATE(ivf_stmask_expand_bwd(dM, A_H, A_W, dsig, b, v.T, gh, gw, H, W, s));
    IVF_PROPAGATE(ivf_stmask_step(raw, sig, dsig, dreg, terms, score, exp_avg, exp_avg_sq,
                                  traj ? traj + (size_t)it * b * 5 : nullptr, b, v.T, gh, gw, first_step + it, lr, beta1,
                                  beta2, eps, s));
  }
  prof_set_iteration(-1);
  return IVF_OK;
}

// Scores of a flattened candidate list, `per` rows for each of b clips (scores [b,per]): per chunk (for_each_chunk)
// stage(first, cnt) writes the rows straight into the input buffer, then forward, then blob_pick of the target score --
// all on one stream, no host synchronisation, no allocation, no scratch beyond `scores`.  The wrappers below give the
// row count and the staging call of each search; a count they refuse never reaches the loop.
template <class Stage>
static inline int run_row_scores(const Backbone& v, int b, long long per, const int* target, float* scores, hipStream_t s,
                                 Stage&& stage) {
  return for_each_chunk(v, b * per, [&](long long first, int cnt) -> int {
    IVF_PROPAGATE(stage(first, cnt));
    IVF_PROPAGATE(v.forward(v.plan, cnt, nullptr, s));
    return blob_pick(v.probs, target, v.K, (int)per, first, cnt, scores, s);
  });
}

// Exhaustive one-blob search (maskType 'combi'): the n candidates of a clip
static inline int run_blob_scores(const Backbone& v, const float* x, int b, const int* target, int max_len, int mode,
                                  float* scores, hipStream_t s) {
  const int n = ivf_blob_count(v.T, max_len);
  if (n < 0) return IVF_ERR_BAD_ARG;
  return run_row_scores(v, b, n, target, scores, s, [&](long long first, int cnt) {
    return ivf_blob_stage(x, b, v.C, v.T, v.HW, max_len, mode, first, cnt, v.in, v.layout, s);
  });
}

// Exhaustive one-box search (maskType 'stcombi', stmask_ops.hip)
static inline int run_box_scores(const Backbone& v, const float* x, int b, const int* target, const float* A_H,
                                 const float* A_W, int gh, int gw, int H, int W, int max_len, int mh, int mw,
                                 float* scores, hipStream_t s) {
  const long long n = ivf_box_count(v.T, max_len, gh, gw, mh, mw);
  if (n < 0) return IVF_ERR_BAD_ARG;
  return run_row_scores(v, b, n, target, scores, s, [&](long long first, int cnt) {
    return ivf_box_stage(x, b, v.C, v.T, H, W, A_H, A_W, gh, gw, max_len, mh, mw, first, cnt, v.in, v.layout, s);
  });
}

// RISE random-mask saliency (rise_ops.hip; an extension): the n masks of a clip
static inline int run_rise_scores(const Backbone& v, const float* x, int b, const int* target, const float* A_H,
                                  const float* A_W, int gt, int gh, int gw, int H, int W, int n, unsigned seed,
                                  unsigned thresh, float* scores, hipStream_t s) {
  return run_row_scores(v, b, n, target, scores, s, [&](long long first, int cnt) {
    return ivf_rise_stage(x, b, v.C, v.T, H, W, A_H, A_W, gt, gh, gw, n, seed, thresh, first, cnt, v.in, v.layout, s);
  });
}

// Shapley value sampling (shapley_ops.hip; an extension): the n * (P + 1) (permutation, prefix) rows of a
// clip, ranks [n,P] the caller's table
static inline int run_shap_scores(const Backbone& v, const float* x, int b, const int* target, const float* A_H,
                                  const float* A_W, int gt, int gh, int gw, int H, int W, int n,
                                  const unsigned short* ranks, float* scores, hipStream_t s) {
  const long long per = (long long)n * ((long long)gt * gh * gw + 1);
  if (per > 0x7fffffffLL) {
    set_error("shap_scores: %lld rows per clip", per);
    return IVF_ERR_BAD_ARG;
  }
  return run_row_scores(v, b, per, target, scores, s, [&](long long first, int cnt) {
    return ivf_shap_stage(x, b, v.C, v.T, H, W, A_H, A_W, gt, gh, gw, n, ranks, first, cnt, v.in, v.layout, s);
  });
}

// Linear surrogates (linsur_ops.hip; an extension): the n sample rows of a clip and its fully frozen row,
// bits [n, ceil(P/32)] the caller's table
static inline int run_lin_scores(const Backbone& v, const float* x, int b, const int* target, const float* A_H,
                                 const float* A_W, int gt, int gh, int gw, int H, int W, int n, const unsigned* bits,
                                 float* scores, hipStream_t s) {
  return run_row_scores(v, b, (long long)n + 1, target, scores, s, [&](long long first, int cnt) {
    return ivf_lin_stage(x, b, v.C, v.T, H, W, A_H, A_W, gt, gh, gw, n, bits, first, cnt, v.in, v.layout, s);
  });
}

// Deletion / insertion curves (curve_ops.hip; an extension): the ncurves * (J + 1) (curve, j) rows of a clip,
// a rank table per clip; chunks cross clip and curve boundaries
static inline int run_curve_scores(const Backbone& v, const float* x, int b, const int* target, const float* A_H,
                                   const float* A_W, int gt, int gh, int gw, int H, int W, const unsigned short* ranks,
                                   int curves, int step, float* scores, hipStream_t s) {
  const long long P = (long long)gt * gh * gw;
  if (curves < 1 || curves > 3 || step < 1 || step > P || P > 4096) {     // what the row count below is made of
    set_error("curve_scores: need curves in 1 .. 3 (got %d) and 1 <= step (%d) <= gt gh gw (%lld) <= 4096", curves, step, P);
    return IVF_ERR_BAD_ARG;
  }
  const long long per = (curves == 3 ? 2 : 1) * ((P + step - 1) / step + 1);
  return run_row_scores(v, b, per, target, scores, s, [&](long long first, int cnt) {
    return ivf_curve_stage(x, b, v.C, v.T, H, W, A_H, A_W, gt, gh, gw, ranks, curves, step, first, cnt, v.in, v.layout, s);
  });
}

// Score-CAM (scorecam_ops.hip; an extension): the nc channel rows of a clip and its baseline row, F
// [b,nc,gt,gh,gw] the freeze planes
static inline int run_scorecam_scores(const Backbone& v, const float* x, int b, const int* target, const float* A_H,
                                      const float* A_W, int gt, int gh, int gw, int H, int W, const float* F, int nc,
                                      int perturb, float* scores, hipStream_t s) {
  return run_row_scores(v, b, (long long)nc + 1, target, scores, s, [&](long long first, int cnt) {
    return ivf_scorecam_stage(x, b, v.C, v.T, H, W, A_H, A_W, gt, gh, gw, F, nc, perturb, first, cnt, v.in, v.layout, s);
  });
}

// ---------------------------------------------------------------- Integrated Gradients (ig_ops.hip)
// An extension without a counterpart in the reference.  Its scratch belongs to the CALLER (ivf_ig_workspace_bytes), so
// no plan's workspace size or carve order moves.
struct IgScratch {
  size_t gsum = 0, rowt = 0, score = 0;

  // byte offsets of the pieces, each 256-byte aligned; returns the total.  per_clip = C * T * HW.
  size_t carve(size_t b, size_t per_clip, size_t K) {
    Bump256 a;
    gsum = a.take(b * per_clip * 4);
    rowt = a.take(b * K * 4);
    score = a.take(b * K * 4);
    return a.top;
  }
};

// Scores of the K path points x0 + alpha[k] (x - x0) of a clip.  scores [b,K].
static inline int run_ig_path_scores(const Backbone& v, const float* x, int b, const int* target, int base_kind,
                                     const float* base, float base_value, const float* alpha, int K, float* scores,
                                     hipStream_t s) {
  return run_row_scores(v, b, K, target, scores, s, [&](long long first, int cnt) {
    return ivf_ig_stage(x, base_kind, base, base_value, alpha, b, v.C, v.T, v.HW, K, first, cnt, v.in, v.layout, s);
  });
}

// Integrated Gradients of b clips: per chunk of the plan's B rows stage -> forward -> backward -> accumulate, then
// finish.  path_scores [b,K] (optional): the scores the backward writes.  `ws`: the caller's
// ivf_ig_workspace_bytes(b, C, T, HW, K) bytes.  One stream, no host synchronisation, no allocation.
static int run_ig(const Backbone& v, const float* x, int b, const int* target, int base_kind, const float* base,
                  float base_value, const float* alpha, const float* w, int K, float* ig_map, float* frames,
                  float* abs_frames, float* total_out, float* path_scores, void* ws, hipStream_t s) {
  IgScratch c;
  const size_t per_clip = (size_t)v.C * v.T * v.HW;
  c.carve((size_t)b, per_clip, (size_t)K);
  float* Gsum = (float*)((char*)ws + c.gsum);
  int* rowt = (int*)((char*)ws + c.rowt);
  float* score = path_scores ? path_scores : (float*)((char*)ws + c.score);
  IVF_CHECK_HIP(hipMemsetAsync(Gsum, 0, (size_t)b * per_clip * 4, s));
  IVF_PROPAGATE(ig_row_targets(target, b, K, rowt, s));
  IVF_PROPAGATE(for_each_chunk(v, (long long)b * K, [&](long long first, int cnt) -> int {
    IVF_PROPAGATE(ivf_ig_stage(x, base_kind, base, base_value, alpha, b, v.C, v.T, v.HW, K, first, cnt, v.in, v.layout, s));
    IVF_PROPAGATE(v.forward(v.plan, cnt, nullptr, s));
    IVF_PROPAGATE(v.backward(v.plan, cnt, rowt + first, score + first, s));
    return ivf_ig_accumulate(v.din, v.layout, w, K, first, cnt, Gsum, b, v.C, v.T, v.HW, s);
  }));
  return ivf_ig_finish(x, base_kind, base, base_value, Gsum, b, v.C, v.T, v.HW, ig_map, frames, abs_frames, total_out, s);
}

// ---------------------------------------------------------------- SmoothGrad / SmoothGrad^2 / VarGrad (smoothgrad_ops.hip)
// An extension without a counterpart in the reference.  Its scratch belongs to the CALLER (ivf_sg_workspace_bytes), so
// no plan's workspace size or carve order moves.
struct SgScratch {
  size_t g1 = 0, g2 = 0, sigma = 0, rowt = 0, score = 0;

  // byte offsets of the pieces, each 256-byte aligned; returns the total.  per_clip = C * T * HW.
  size_t carve(size_t b, size_t per_clip, size_t n) {
    Bump256 a;
    g1 = a.take(b * per_clip * 4);
    g2 = a.take(b * per_clip * 4);
    sigma = a.take(b * 4);
    rowt = a.take(b * n * 4);
    score = a.take(b * n * 4);
    return a.top;
  }
};

// The two gradient moments of b clips under n noisy samples each: range -> zero G1 / G2 -> per-row targets, then per
// chunk of the plan's B rows stage -> forward -> backward -> accumulate, then finish.  sample_scores [b,n] and sigma [b]
// (both optional): the scores the backward writes and the noise scale of each clip.  `ws`: the caller's
// ivf_sg_workspace_bytes(b, C, T, HW, n) bytes.  One stream, no host synchronisation, no allocation.
static int run_smoothgrad(const Backbone& v, const float* x, int b, const int* target, int n, float level, unsigned seed,
                          float* sg_map, float* sq_map, float* var_map, float* sg_frames, float* sq_frames,
                          float* var_frames, float* sample_scores, float* sigma_out, void* ws, hipStream_t s) {
  SgScratch c;
  const size_t per_clip = (size_t)v.C * v.T * v.HW;
  c.carve((size_t)b, per_clip, (size_t)n);
  float *G1 = (float*)((char*)ws + c.g1), *G2 = (float*)((char*)ws + c.g2);
  float* sigma = sigma_out ? sigma_out : (float*)((char*)ws + c.sigma);
  int* rowt = (int*)((char*)ws + c.rowt);
  float* score = sample_scores ? sample_scores : (float*)((char*)ws + c.score);
  IVF_PROPAGATE(ivf_sg_range(x, b, v.C, v.T, v.HW, level, sigma, s));
  IVF_CHECK_HIP(hipMemsetAsync(G1, 0, (size_t)b * per_clip * 4, s));
  IVF_CHECK_HIP(hipMemsetAsync(G2, 0, (size_t)b * per_clip * 4, s));
  IVF_PROPAGATE(ig_row_targets(target, b, n, rowt, s));
  IVF_PROPAGATE(for_each_chunk(v, (long long)b * n, [&](long long first, int cnt) -> int {
    IVF_PROPAGATE(ivf_sg_stage(x, sigma, b, v.C, v.T, v.HW, n, seed, first, cnt, v.in, v.layout, s));
    IVF_PROPAGATE(v.forward(v.plan, cnt, nullptr, s));
    IVF_PROPAGATE(v.backward(v.plan, cnt, rowt + first, score + first, s));
    return ivf_sg_accumulate(v.din, v.layout, n, first, cnt, G1, G2, b, v.C, v.T, v.HW, s);
  }));
  return ivf_sg_finish(G1, G2, n, b, v.C, v.T, v.HW, sg_map, sq_map, var_map, sg_frames, sq_frames, var_frames, s);
}

}  // namespace ivf
