// Integrated Gradients for video, an EXTENSION with no counterpart in the reference:
// the path x(alpha) = x0 + alpha (x - x0) from a baseline clip x0 to the clip x, K nodes alpha[k] with weights w[k].
//
//   rows of the flattened (clip, node) list, staged straight into a plan's input buffer      (ivf_ig_stage)
//   Gsum[b,c,t,px] = sum_k w[k] d score / d x(alpha[k]), k ascending, fmaf from +0.0          (ivf_ig_accumulate)
//   A = (x - x0) Gsum;  ig_map = sum_c A;  frames = sum_px ig_map;  abs_frames = sum_px sum_c |A|;
//   total = sum_t frames                                                                       (ivf_ig_finish)
//
// All of it is HBM-bound work beside the network's forward and backward.  No float atomics anywhere: every element of
// Gsum has one owner thread that walks its clip's rows in ascending k, and every reduction has a fixed order, so a
// clip's results depend neither on the batch it ran in nor on how the b K rows were cut into chunks.
#include <type_traits>

#include "search_driver.h"

namespace ivf {

// base_kind: where x0 comes from
constexpr int IG_BASE_FROZEN = 0;     // frame 0 of the row's own clip at every frame (mask.py:123-128)
constexpr int IG_BASE_CONSTANT = 1;   // base_value everywhere
constexpr int IG_BASE_CLIP = 2;       // an explicit [b,C,T,HW] tensor

// x(alpha) with one rounding for the difference and one for the fused multiply-add: exact where x == x0 (the product
// is a signed zero) and at alpha == 0, and within 3 ulp-halves of max(|x|, |x0|) for alpha in [0,1] (tests/ig_refs.py).
__device__ __forceinline__ float ig_point(float xv, float x0, float a) { return fmaf(a, xv - x0, x0); }

// x0 of element (c, u, px) of clip `xc` (= x + clip * C*T*HW); bc = base + clip * C*T*HW (IG_BASE_CLIP only)
__device__ __forceinline__ float ig_base(const float* __restrict__ xc, const float* __restrict__ bc, int kind,
                                         float value, int c, int u, int T, int HW, int px) {
  if (kind == IG_BASE_FROZEN) return xc[(size_t)c * T * HW + px];
  if (kind == IG_BASE_CONSTANT) return value;
  return bc[((size_t)c * T + u) * HW + px];
}

// ---------------------------------------------------------------- stage
// 16-byte channels-last pixels (C <= 4): one thread per (row, pixel), one 16-byte store per frame, pad lanes +0.0 (the
// layout blob_stage_cl4_kernel writes); row j = node (first + j) % K of clip (first + j) / K.
__global__ __launch_bounds__(256) void ig_stage_cl4_kernel(const float* __restrict__ x, const float* __restrict__ base,
                                                           int kind, float value, const float* __restrict__ alpha, int C,
                                                           int T, int HW, int K, long long first, int count,
                                                           float* __restrict__ p) {
  size_t total = (size_t)count * HW;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int px = i % HW;
    int j = i / HW;
    long long g = first + j;
    int clip = (int)(g / K);
    const float a = alpha[(int)(g % K)];
    const float* xc = x + (size_t)clip * C * T * HW;
    const float* bc = kind == IG_BASE_CLIP ? base + (size_t)clip * C * T * HW : nullptr;
    float x0[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C && kind != IG_BASE_CLIP) x0[c] = ig_base(xc, bc, kind, value, c, 0, T, HW, px);
    for (int u = 0; u < T; ++u) {
      float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) {
          const float b0 = kind == IG_BASE_CLIP ? bc[((size_t)c * T + u) * HW + px] : x0[c];
          v[c] = ig_point(xc[((size_t)c * T + u) * HW + px], b0, a);
        }
      *reinterpret_cast<float4*>(p + (((size_t)j * T + u) * HW + px) * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// NCTHW: one thread per (row, channel, 4-pixel quad) when HW % 4 == 0 (16-byte loads and stores), else per pixel
template <int V>
__global__ __launch_bounds__(256) void ig_stage_ncthw_kernel(const float* __restrict__ x, const float* __restrict__ base,
                                                             int kind, float value, const float* __restrict__ alpha,
                                                             int C, int T, int HW, int K, long long first, int count,
                                                             float* __restrict__ p) {
  using vec = typename std::conditional<V == 4, float4, float>::type;
  const int HWv = HW / V;
  size_t total = (size_t)count * C * HWv;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int q = i % HWv;
    int c = (i / HWv) % C;
    int j = i / ((size_t)HWv * C);
    long long g = first + j;
    int clip = (int)(g / K);
    const float a = alpha[(int)(g % K)];
    const vec* xc = reinterpret_cast<const vec*>(x + ((size_t)clip * C + c) * T * HW) + q;
    const vec* bc = kind == IG_BASE_CLIP ? reinterpret_cast<const vec*>(base + ((size_t)clip * C + c) * T * HW) + q : nullptr;
    vec* pc = reinterpret_cast<vec*>(p + ((size_t)j * C + c) * T * HW) + q;
    vec x0{};
    if (kind == IG_BASE_FROZEN) x0 = xc[0];
    for (int u = 0; u < T; ++u) {
      const vec xv = xc[(size_t)u * HWv];
      if (kind == IG_BASE_CLIP) x0 = bc[(size_t)u * HWv];
      vec v;
      if constexpr (V == 4) {
        if (kind == IG_BASE_CONSTANT) x0 = make_float4(value, value, value, value);
        v = make_float4(ig_point(xv.x, x0.x, a), ig_point(xv.y, x0.y, a), ig_point(xv.z, x0.z, a),
                        ig_point(xv.w, x0.w, a));
      } else {
        if (kind == IG_BASE_CONSTANT) x0 = value;
        v = ig_point(xv, x0, a);
      }
      pc[(size_t)u * HWv] = v;
    }
  }
}

// ---------------------------------------------------------------- accumulate
// The window holds rows [first, first + count) of the (clip, node) list, i.e. clips c0 = first / K .. (first+count-1) / K.
// NCTHW: one thread per element (clip, c, t, px) of those clips; it walks the window's rows of its clip in ascending k.
__global__ __launch_bounds__(256) void ig_accumulate_ncthw_kernel(const float* __restrict__ din,
                                                                  const float* __restrict__ w, int K, long long first,
                                                                  int count, int c0, int nclips, size_t per_clip,
                                                                  float* __restrict__ Gsum) {
  size_t total = (size_t)nclips * per_clip;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i % per_clip;
    const int clip = c0 + (int)(i / per_clip);
    long long lo = (long long)clip * K - first, hi = lo + K;   // rows of this clip, relative to the window
    const int k0 = lo < 0 ? (int)-lo : 0;
    if (lo < 0) lo = 0;
    if (hi > count) hi = count;
    float acc = Gsum[(size_t)clip * per_clip + e];
    for (long long j = lo; j < hi; ++j) acc = fmaf(w[k0 + (int)(j - lo)], din[(size_t)j * per_clip + e], acc);
    Gsum[(size_t)clip * per_clip + e] = acc;
  }
}

// 16-byte channels-last rows [count,T,HW,4]: one thread per pixel (clip, t, px); one 16-byte load per row serves the C
// channels, the pad lanes of din are never read into the arithmetic.
__global__ __launch_bounds__(256) void ig_accumulate_cl4_kernel(const float* __restrict__ din, const float* __restrict__ w,
                                                                int K, long long first, int count, int c0, int nclips,
                                                                int C, int T, int HW, float* __restrict__ Gsum) {
  const size_t THW = (size_t)T * HW;
  size_t total = (size_t)nclips * THW;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i % THW;
    const int clip = c0 + (int)(i / THW);
    long long lo = (long long)clip * K - first, hi = lo + K;
    const int k0 = lo < 0 ? (int)-lo : 0;
    if (lo < 0) lo = 0;
    if (hi > count) hi = count;
    float* gp = Gsum + (size_t)clip * C * THW + e;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) acc[c] = gp[(size_t)c * THW];
    for (long long j = lo; j < hi; ++j) {
      const float4 g = *reinterpret_cast<const float4*>(din + ((size_t)j * THW + e) * 4);
      const float wk = w[k0 + (int)(j - lo)];
      const float gv[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) acc[c] = fmaf(wk, gv[c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) gp[(size_t)c * THW] = acc[c];
  }
}

// ---------------------------------------------------------------- finish
// One workgroup per (clip, frame): every thread takes the pixels px = tid, tid + 256, ... in that order (ig_map is
// written on the way), then a wave64 shuffle tree, then the four waves in order, as stmask_reg_kernel sums.
__global__ __launch_bounds__(256) void ig_finish_kernel(const float* __restrict__ x, const float* __restrict__ base,
                                                        int kind, float value, const float* __restrict__ Gsum, int C,
                                                        int T, int HW, float* __restrict__ ig_map,
                                                        float* __restrict__ frames, float* __restrict__ abs_frames) {
  const int t = blockIdx.x % T, b = blockIdx.x / T;
  const float* xc = x + (size_t)b * C * T * HW;
  const float* bc = kind == IG_BASE_CLIP ? base + (size_t)b * C * T * HW : nullptr;
  const float* gc = Gsum + (size_t)b * C * T * HW;
  float sum = 0.f, asum = 0.f;
  for (int px = threadIdx.x; px < HW; px += 256) {
    float m = 0.f, am = 0.f;
    for (int c = 0; c < C; ++c) {
      const size_t e = ((size_t)c * T + t) * HW + px;
      const float A = (xc[e] - ig_base(xc, bc, kind, value, c, t, T, HW, px)) * gc[e];
      m += A;
      am += fabsf(A);
    }
    ig_map[((size_t)b * T + t) * HW + px] = m;
    sum += m;
    asum += am;
  }
  __shared__ float red[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float v[2] = {sum, asum};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    if (lane == 0) red[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int k = threadIdx.x;
    const float r = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    (k == 0 ? frames : abs_frames)[(size_t)b * T + t] = r;
  }
}

// total[b] = sum_t frames[b,t], t ascending
__global__ void ig_total_kernel(const float* __restrict__ frames, int B, int T, float* __restrict__ total) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float s = 0.f;
  for (int t = 0; t < T; ++t) s += frames[(size_t)b * T + t];
  total[b] = s;
}

// rowt[g] = target[g / K]: the per-row targets a plan's backward takes
__global__ void ig_row_targets_kernel(const int* __restrict__ target, int K, long long total, int* __restrict__ rowt) {
  long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (g < total) rowt[g] = target[g / K];
}

int ig_row_targets(const int* target, int b, int K, int* rowt, hipStream_t s) {
  const long long total = (long long)b * K;
  hipLaunchKernelGGL(ig_row_targets_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, target, K, total, rowt);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

static bool ig_base_ok(int kind, const float* base) {
  return kind == IG_BASE_FROZEN || kind == IG_BASE_CONSTANT || (kind == IG_BASE_CLIP && base);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace ivf

using namespace ivf;

extern "C" size_t ivf_ig_workspace_bytes(int b, int C, int T, int HW, int K) {
  if (b <= 0 || C <= 0 || T <= 0 || HW <= 0 || K <= 0) {
    set_error("ig_workspace_bytes: bad dims");
    return 0;
  }
  return IgScratch().carve((size_t)b, (size_t)C * T * HW, (size_t)K);
}

extern "C" int ivf_ig_stage(const float* x, int base_kind, const float* base, float base_value, const float* alpha, int b,
                            int C, int T, int HW, int K, long long first, int count, float* out, int layout,
                            ivf_stream_t stream) {
  IVF_CHECK_ARG(x && alpha && out, "ig_stage: null pointer");
  IVF_CHECK_ARG(b > 0 && C > 0 && T > 0 && HW > 0 && K > 0, "ig_stage: bad dims");
  IVF_CHECK_ARG(ig_base_ok(base_kind, base), "ig_stage: base_kind must be 0 (frozen), 1 (constant) or 2 (clip, base given)");
  IVF_CHECK_ARG(first >= 0 && count > 0 && first + count <= (long long)b * K,
                "ig_stage: rows [%lld, %lld) outside the %lld path points of %d clips", first, first + count,
                (long long)b * K, b);
  IVF_CHECK_ARG(layout == 0 || (layout == 4 && C <= 4),
                "ig_stage: layout must be 0 (NCTHW) or 4 (16-byte channels-last, C <= 4)");
  hipStream_t s = (hipStream_t)stream;
  if (layout == 4) {
    IVF_CHECK_ARG(aligned16(out), "ig_stage: channels-last output must be 16-byte aligned");
    hipLaunchKernelGGL(ig_stage_cl4_kernel, dim3(grid_for((size_t)count * HW, 256, 2048)), dim3(256), 0, s, x, base,
                       base_kind, base_value, alpha, C, T, HW, K, first, count, out);
  } else if (HW % 4 == 0 && aligned16(x) && aligned16(out) && (base_kind != IG_BASE_CLIP || aligned16(base))) {
    hipLaunchKernelGGL(ig_stage_ncthw_kernel<4>, dim3(grid_for((size_t)count * C * HW / 4, 256, 2048)), dim3(256), 0, s, x,
                       base, base_kind, base_value, alpha, C, T, HW, K, first, count, out);
  } else {
    hipLaunchKernelGGL(ig_stage_ncthw_kernel<1>, dim3(grid_for((size_t)count * C * HW, 256, 2048)), dim3(256), 0, s, x,
                       base, base_kind, base_value, alpha, C, T, HW, K, first, count, out);
  }
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_ig_accumulate(const float* din, int layout, const float* w, int K, long long first, int count,
                                 float* Gsum, int b, int C, int T, int HW, ivf_stream_t stream) {
  IVF_CHECK_ARG(din && w && Gsum, "ig_accumulate: null pointer");
  IVF_CHECK_ARG(b > 0 && C > 0 && T > 0 && HW > 0 && K > 0, "ig_accumulate: bad dims");
  IVF_CHECK_ARG(first >= 0 && count > 0 && first + count <= (long long)b * K,
                "ig_accumulate: rows [%lld, %lld) outside the %lld path points of %d clips", first, first + count,
                (long long)b * K, b);
  IVF_CHECK_ARG(layout == 0 || (layout == 4 && C <= 4),
                "ig_accumulate: layout must be 0 (NCTHW) or 4 (16-byte channels-last, C <= 4)");
  const int c0 = (int)(first / K), nclips = (int)((first + count - 1) / K) - c0 + 1;
  hipStream_t s = (hipStream_t)stream;
  if (layout == 4) {
    IVF_CHECK_ARG(aligned16(din), "ig_accumulate: channels-last gradient must be 16-byte aligned");
    hipLaunchKernelGGL(ig_accumulate_cl4_kernel, dim3(grid_for((size_t)nclips * T * HW, 256, 4096)), dim3(256), 0, s, din, w,
                       K, first, count, c0, nclips, C, T, HW, Gsum);
  } else {
    const size_t per_clip = (size_t)C * T * HW;
    hipLaunchKernelGGL(ig_accumulate_ncthw_kernel, dim3(grid_for((size_t)nclips * per_clip, 256, 4096)), dim3(256), 0, s,
                       din, w, K, first, count, c0, nclips, per_clip, Gsum);
  }
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_ig_finish(const float* x, int base_kind, const float* base, float base_value, const float* Gsum, int b,
                             int C, int T, int HW, float* ig_map, float* frames, float* abs_frames, float* total,
                             ivf_stream_t stream) {
  IVF_CHECK_ARG(x && Gsum && ig_map && frames && abs_frames && total, "ig_finish: null pointer");
  IVF_CHECK_ARG(b > 0 && C > 0 && T > 0 && HW > 0 && (long long)b * T <= 0x7fffffffLL, "ig_finish: bad dims");
  IVF_CHECK_ARG(ig_base_ok(base_kind, base), "ig_finish: base_kind must be 0 (frozen), 1 (constant) or 2 (clip, base given)");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ig_finish_kernel, dim3(b * T), dim3(256), 0, s, x, base, base_kind, base_value, Gsum, C, T, HW, ig_map,
                     frames, abs_frames);
  IVF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ig_total_kernel, dim3(cdiv(b, 64)), dim3(64), 0, s, frames, b, T, total);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}
