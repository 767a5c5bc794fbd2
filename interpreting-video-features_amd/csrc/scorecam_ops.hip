// Score-CAM for video (Wang et al., CVPR-W 2020), an EXTENSION with no counterpart in the reference: the
// activation-map method without a gradient.  A target layer gives channel-major activations A [nc,gt,gh,gw] per clip;
// every channel is normalised to a freeze plane F_k = (hi - A_k) / (hi - lo) in [0, 1] (0 where the channel fires
// most), expanded to the clip as the spacetime masks are and applied to the input, one forward per channel plus one
// for the baseline row; the channel's weight is what its row scores above the baseline, the map relu(sum_k w_k A_k).
//
// What is new beside grid_stage.h is that a row's mask is dense and real-valued: the row's plane is parked in LDS next
// to the A_W columns, and per pixel and temporal cell
//   tmp[i] = sum_j F[kt,i,j] * A_W[x,j]      (j ascending)
//   M      = sum_i A_H[y,i] * tmp[i]         (i ascending)
// every partial sum rounded as stmask_expand_fwd_kernel rounds it (no contraction: a multiply and an add each), then
// the recurrence expression of ivf_stfreeze_fwd.  Nothing is skipped: the sums are the dense ones.
#include "grid_stage.h"

namespace ivf {

constexpr int SC_MAX_CELLS = 8192;      // a row's plane in LDS: 32 KiB beside the 32 KiB of A_W columns

// ---------------------------------------------------------------- normalise
// One workgroup per (clip, channel): min / max over the plane (order-free, so exact; a zero result is written as +0.0
// whatever the signs of the zeros met on the way), then F.  A NaN anywhere makes lo = hi = NaN.
__global__ __launch_bounds__(256) void scorecam_normalise_kernel(const float* __restrict__ A, int cells,
                                                                 float* __restrict__ lo_out, float* __restrict__ hi_out,
                                                                 int* __restrict__ valid_out, float* __restrict__ F) {
  __shared__ float s_lo[4], s_hi[4];
  __shared__ int s_nan[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* a = A + (size_t)blockIdx.x * cells;
  float lo = INFINITY, hi = -INFINITY;
  int nan = 0;
  for (int c = tid; c < cells; c += 256) {
    const float v = a[c];
    nan |= v != v;
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_down(lo, o, 64));
    hi = fmaxf(hi, __shfl_down(hi, o, 64));
    nan |= __shfl_down(nan, o, 64);
  }
  if (lane == 0) {
    s_lo[wave] = lo;
    s_hi[wave] = hi;
    s_nan[wave] = nan;
  }
  __syncthreads();
  lo = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3])) + 0.f;
  hi = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3])) + 0.f;
  if (s_nan[0] | s_nan[1] | s_nan[2] | s_nan[3]) lo = hi = __builtin_nanf("");
  const bool valid = fabsf(lo) < INFINITY && fabsf(hi) < INFINITY && hi > lo;
  if (tid == 0) {
    lo_out[blockIdx.x] = lo;
    hi_out[blockIdx.x] = hi;
    valid_out[blockIdx.x] = valid ? 1 : 0;
  }
  const float range = hi - lo;
  float* f = F + (size_t)blockIdx.x * cells;
  for (int c = tid; c < cells; c += 256) f[c] = valid ? (hi - a[c]) / range : 1.f;
}

// ---------------------------------------------------------------- staging
// One workgroup per (row, 256 pixels), as grid_stage.h: the row's plane goes into LDS once (every lane reads the same
// word of it: a broadcast), every thread parks row x of A_W in its own LDS column (aw[j * 256 + tid]: a wave reads 64
// consecutive words, no bank conflict).  M is computed once on entering a temporal cell.  A baseline row touches no
// LDS and no mask arithmetic.
struct ScRow {
  int clip, mode;        // mode: perturb (0 freeze, 1 blank) + 2 for the baseline row
  const float* plane;    // F of the row's channel (unused by a baseline row)
};

__device__ __forceinline__ ScRow sc_row(long long r, const float* __restrict__ F, int nc, int cells, int perturb) {
  const int clip = (int)(r / (nc + 1)), k = (int)(r % (nc + 1));
  if (k == nc) return {clip, perturb + 2, F};
  return {clip, perturb, F + ((size_t)clip * nc + k) * cells};
}

struct ScLds {
  const float *plane, *aw;
};

__device__ __forceinline__ ScLds sc_fill_lds(float* lds, const ScRow& q, const float* __restrict__ AW, int cells, int gw,
                                             int x) {
  const int tid = threadIdx.x;
  if (q.mode < 2) {      // the same for the whole workgroup
    for (int c = tid; c < cells; c += 256) lds[c] = q.plane[c];
    for (int j = 0; j < gw; ++j) lds[cells + j * 256 + tid] = AW[(size_t)x * gw + j];
  }
  __syncthreads();
  return {lds, lds + cells};
}

// M[y,x] of the row's mask on the frames of temporal cell kt; A_H row y is read through the cache
__device__ __forceinline__ float sc_mask_at(const ScLds& l, const float* __restrict__ AHy, int gh, int gw, int kt) {
  const float* f = l.plane + kt * gh * gw;
  const float* aw = l.aw + threadIdx.x;
  float m = 0.f;
  for (int i = 0; i < gh; ++i) {
    float t = 0.f;
    for (int j = 0; j < gw; ++j) t += f[i * gw + j] * aw[j * 256];
    m += AHy[i] * t;
  }
  return m;
}

// frame u of a row from the clip's frame xv and the row's frame u - 1
__device__ __forceinline__ float sc_frame(int mode, int u, float m, float xv, float prev) {
  if (mode == 0) return u ? (1.f - m) * xv + m * prev : xv;
  if (mode == 1) return (1.f - m) * xv;
  if (mode == 2) return u ? prev : xv;      // M == 1: every frame is frame 0
  return 0.f;                                // M == 1 on a zero baseline
}

// 16-byte channels-last pixels (C <= 4), the scan of grid_stage_cl4_kernel: with TT > 0 (T == TT) the 16 frames of a
// piece are requested before the scan goes over them.
template <int TT>   // 0, or a multiple of 16
__global__ __launch_bounds__(256) void scorecam_stage_cl4_kernel(const float* __restrict__ x, const float* __restrict__ AH,
                                                                 const float* __restrict__ AW, const float* __restrict__ F,
                                                                 float* __restrict__ p, int C, int Trun, int W, int HW,
                                                                 Grid3 g, int nc, int perturb, long long first) {
  extern __shared__ float sc_lds[];
  const int row = blockIdx.y, T = TT > 0 ? TT : Trun, cells = g.gt * g.gh * g.gw;
  const ScRow q = sc_row(first + row, F, nc, cells, perturb);
  const int pxu = blockIdx.x * 256 + threadIdx.x;
  const int px = min(pxu, HW - 1);          // threads past the end stage LDS for a valid pixel, then leave
  const ScLds l = sc_fill_lds(sc_lds, q, AW, cells, g.gw, px % W);
  if (pxu >= HW) return;
  const float* AHy = AH + (size_t)(px / W) * g.gh;
  const float* xc = x + (size_t)q.clip * C * T * HW + px;
  float* pr = p + ((size_t)row * T * HW + px) * 4;
  float prev[4] = {0.f, 0.f, 0.f, 0.f};
  int cur = -1;
  float m = 0.f;
  if constexpr (TT > 0) {
#pragma unroll 1
    for (int u0 = 0; u0 < TT; u0 += 16) {
      float xv[4][16];
#pragma unroll
      for (int ch = 0; ch < 4; ++ch)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          xv[ch][j] = 0.f;
          if (ch < C) xv[ch][j] = xc[((size_t)ch * TT + u0 + j) * HW];
        }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int u = u0 + j, kt = (u * g.gt) / TT;
        if (kt != cur && q.mode < 2) {
          cur = kt;
          m = sc_mask_at(l, AHy, g.gh, g.gw, kt);
        }
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
          if (ch < C) {
            v[ch] = sc_frame(q.mode, u, m, xv[ch][j], prev[ch]);
            prev[ch] = v[ch];
          }
        *reinterpret_cast<float4*>(pr + (size_t)u * HW * 4) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  } else {
    for (int u = 0; u < T; ++u) {
      const int kt = (u * g.gt) / T;
      if (kt != cur && q.mode < 2) {
        cur = kt;
        m = sc_mask_at(l, AHy, g.gh, g.gw, kt);
      }
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      for (int ch = 0; ch < C; ++ch) {
        float xv = xc[((size_t)ch * T + u) * HW];
        v[ch] = sc_frame(q.mode, u, m, xv, prev[ch]);
        prev[ch] = v[ch];
      }
      *reinterpret_cast<float4*>(pr + (size_t)u * HW * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// NCTHW: channel after channel, as grid_stage_ncthw_kernel (the mask value is the pixel's, not the channel's; it is
// recomputed per channel from LDS)
__global__ __launch_bounds__(256) void scorecam_stage_ncthw_kernel(const float* __restrict__ x, const float* __restrict__ AH,
                                                                   const float* __restrict__ AW, const float* __restrict__ F,
                                                                   float* __restrict__ p, int C, int T, int W, int HW,
                                                                   Grid3 g, int nc, int perturb, long long first) {
  extern __shared__ float sc_lds[];
  const int row = blockIdx.y, cells = g.gt * g.gh * g.gw;
  const ScRow q = sc_row(first + row, F, nc, cells, perturb);
  const int pxu = blockIdx.x * 256 + threadIdx.x;
  const int px = min(pxu, HW - 1);
  const ScLds l = sc_fill_lds(sc_lds, q, AW, cells, g.gw, px % W);
  if (pxu >= HW) return;
  const float* AHy = AH + (size_t)(px / W) * g.gh;
  for (int ch = 0; ch < C; ++ch) {
    const float* xp = x + ((size_t)q.clip * C + ch) * T * HW + px;
    float* pp = p + ((size_t)row * C + ch) * T * HW + px;
    float prev = 0.f, m = 0.f;
    int cur = -1;
    for (int u = 0; u < T; ++u) {
      const int kt = (u * g.gt) / T;
      if (kt != cur && q.mode < 2) {
        cur = kt;
        m = sc_mask_at(l, AHy, g.gh, g.gw, kt);
      }
      float xv = xp[(size_t)u * HW];
      float v = sc_frame(q.mode, u, m, xv, prev);
      prev = v;
      pp[(size_t)u * HW] = v;
    }
  }
}

// ---------------------------------------------------------------- reduction
// One thread per clip walks the channels in ascending k: d_k = s_k - s_nc, a channel counts when it is valid and d_k is
// not NaN.  weights_kind 0: w_k = d_k.  1: w_k = expf(d_k - d_max) / sum over the counting channels (k ascending).
__global__ __launch_bounds__(64) void scorecam_weights_kernel(const float* __restrict__ scores, const int* __restrict__ valid,
                                                              int B, int nc, int kind, float* __restrict__ w) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const float* s = scores + (size_t)b * (nc + 1);
  const int* ok = valid + (size_t)b * nc;
  float* wb = w + (size_t)b * nc;
  const float base = s[nc];
  if (kind == 0) {
    for (int k = 0; k < nc; ++k) {
      const float d = s[k] - base;
      wb[k] = (ok[k] && d == d) ? d : 0.f;
    }
    return;
  }
  float dmax = -INFINITY;
  for (int k = 0; k < nc; ++k) {
    const float d = s[k] - base;
    if (ok[k] && d == d) dmax = fmaxf(dmax, d);
  }
  float sum = 0.f;
  for (int k = 0; k < nc; ++k) {
    const float d = s[k] - base;
    if (ok[k] && d == d) sum += expf(d - dmax);
  }
  for (int k = 0; k < nc; ++k) {
    const float d = s[k] - base;
    wb[k] = (ok[k] && d == d) ? expf(d - dmax) / sum : 0.f;
  }
}

// One thread per (clip, position), k ascending, a multiply and an add each; a channel of weight 0 adds nothing (so the
// non-finite plane of a channel that is not valid never reaches the map).  Position is A's contiguous axis.
__global__ __launch_bounds__(256) void scorecam_cam_kernel(const float* __restrict__ A, const float* __restrict__ w, int B,
                                                           int nc, int cells, float* __restrict__ cam) {
  const size_t e = blockIdx.x * (size_t)256 + threadIdx.x;
  if (e >= (size_t)B * cells) return;
  const int b = (int)(e / cells), pos = (int)(e - (size_t)b * cells);
  const float* a = A + (size_t)b * nc * cells + pos;
  const float* wb = w + (size_t)b * nc;
  float acc = 0.f;
  for (int k = 0; k < nc; ++k) {
    const float wk = wb[k];
    if (wk != 0.f) acc += wk * a[(size_t)k * cells];
  }
  cam[e] = fmaxf(acc, 0.f);
}

}  // namespace ivf

using namespace ivf;

extern "C" int ivf_scorecam_normalise(const float* A, int b, int nc, int cells, float* lo, float* hi, int* valid, float* F,
                                      ivf_stream_t stream) {
  IVF_CHECK_ARG(A && lo && hi && valid && F, "scorecam_normalise: null pointer");
  IVF_CHECK_ARG(b > 0 && nc > 0 && (long long)b * nc <= 0x7fffffffLL, "scorecam_normalise: bad batch %d or channel count %d",
                b, nc);
  IVF_CHECK_ARG(cells >= 1 && cells <= SC_MAX_CELLS, "scorecam_normalise: need 1 <= cells (%d) <= %d", cells, SC_MAX_CELLS);
  hipLaunchKernelGGL(scorecam_normalise_kernel, dim3(b * nc), dim3(256), 0, (hipStream_t)stream, A, cells, lo, hi, valid, F);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_scorecam_stage(const float* x, int b, int C, int T, int H, int W, const float* A_H, const float* A_W,
                                  int gt, int gh, int gw, const float* F, int nc, int perturb, long long first, int count,
                                  float* p, int out_cpad, ivf_stream_t stream) {
  const GridStageArgs a{"scorecam_stage", x, b, C, T, H, W, A_H, A_W, {gt, gh, gw}, first, count, p, out_cpad, stream};
  IVF_PROPAGATE(grid_stage_check(a, F != nullptr, SC_MAX_CELLS));
  IVF_CHECK_ARG(nc > 0, "scorecam_stage: bad channel count %d", nc);
  IVF_CHECK_ARG(perturb == 0 || perturb == 1, "scorecam_stage: perturb must be 0 (freeze) or 1 (blank), got %d", perturb);
  const long long total = (long long)b * (nc + 1);
  IVF_CHECK_ARG(first >= 0 && count > 0 && count <= 65535 && first + count <= total,
                "scorecam_stage: rows [%lld, %lld) outside the %lld rows of %d clips (at most 65535 rows a call)", first,
                first + count, total, b);
  IVF_CHECK_ARG(out_cpad == 0 || (out_cpad == 4 && C <= 4),
                "scorecam_stage: out_cpad must be 0 (NCTHW) or 4 (16-byte channels-last, C <= 4)");
  IVF_CHECK_ARG(out_cpad == 0 || ((uintptr_t)p & 15) == 0, "scorecam_stage: the channels-last buffer is not 16-byte aligned");
  const int HW = H * W;
  const size_t lds = ((size_t)gt * gh * gw + (size_t)gw * 256) * 4;      // at most 32 + 32 KiB
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(cdiv(HW, 256), count), block(256);
  if (out_cpad == 0)
    hipLaunchKernelGGL(scorecam_stage_ncthw_kernel, grid, block, lds, s, x, A_H, A_W, F, p, C, T, W, HW, a.g, nc, perturb,
                       first);
  else
    with_frames_exact(T, [&](auto TT) {
      hipLaunchKernelGGL((scorecam_stage_cl4_kernel<TT>), grid, block, lds, s, x, A_H, A_W, F, p, C, T, W, HW, a.g, nc,
                         perturb, first);
    });
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_scorecam_reduce(const float* scores, const float* A, const int* valid, int b, int nc, int cells,
                                   int weights_kind, float* weights_out, float* cam_out, ivf_stream_t stream) {
  IVF_CHECK_ARG(scores && A && valid && weights_out && cam_out, "scorecam_reduce: null pointer");
  IVF_CHECK_ARG(b > 0 && nc > 0, "scorecam_reduce: bad batch %d or channel count %d", b, nc);
  IVF_CHECK_ARG(cells >= 1 && cells <= SC_MAX_CELLS, "scorecam_reduce: need 1 <= cells (%d) <= %d", cells, SC_MAX_CELLS);
  IVF_CHECK_ARG(weights_kind == 0 || weights_kind == 1,
                "scorecam_reduce: weights_kind must be 0 (increase) or 1 (softmax), got %d", weights_kind);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(scorecam_weights_kernel, dim3(cdiv(b, 64)), dim3(64), 0, s, scores, valid, b, nc, weights_kind,
                     weights_out);
  IVF_CHECK_LAUNCH();
  hipLaunchKernelGGL(scorecam_cam_kernel, dim3(cdiv((long long)b * cells, 256)), dim3(256), 0, s, A, weights_out, b, nc,
                     cells, cam_out);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}
