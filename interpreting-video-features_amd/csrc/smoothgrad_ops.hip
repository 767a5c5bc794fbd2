// SmoothGrad, SmoothGrad^2 and VarGrad for video (Smilkov et al. 2017; Hooker et al. 2019), an EXTENSION with no
// counterpart in the reference: n noisy copies x + sigma z_k of a clip, one forward and one backward each,
// and per input element the first two moments of d score / d input over the samples.
//
//   z(seed, k, e), e = (c T + t) HW + px the NCTHW index inside one clip: the same for every clip and either staged
//   layout, regenerated from a counter-based hash wherever it is needed, never stored                  (sg_z)
//   sigma[clip] = level (max x_clip - min x_clip)                                                       (ivf_sg_range)
//   rows of the flattened (clip, sample) list, p = fmaf(sigma, z, x), straight into a plan's input      (ivf_sg_stage)
//   G1 = G1 + g, G2 = fmaf(g, g, G2) over the samples, k ascending, from +0.0                           (ivf_sg_accumulate)
//   sg_map = sum_c |G1 / n|, sq_map = sum_c G2 / n, var_map = sum_c (G2 - G1 (G1 / n)) / (n - 1), and their sums over
//   the pixels of a frame                                                                                (ivf_sg_finish)
//
// All of it is HBM-bound work beside the network's forward and backward, except the staging, which pays two hashes and
// three transcendentals per element and requests its frames ahead of that arithmetic.  No float atomics anywhere: every
// element of G1 / G2 has one owner thread that walks its clip's rows in ascending k, min and max do not depend on the
// order, and every sum has a fixed order, so a clip's results depend neither on the batch it ran in nor on how the
// b n rows were cut into chunks.
#include <type_traits>

#include "search_driver.h"

namespace ivf {

// MurmurHash3's finaliser, as grid_stage.h has it (restated: the two translation units share no header for it)
__device__ __forceinline__ unsigned sg_fmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
// the part of the hash that belongs to the sample (= rise_key)
__device__ __forceinline__ unsigned sg_key(unsigned seed, int k) { return sg_fmix32(seed + 0x9E3779B9u * (unsigned)(k + 1)); }

// One standard normal per (key, element), Box-Muller without pairing: a = RISE's u(seed, k, c) with e for c gives
// u1 = (2 (a >> 9) + 1) 2^-24 in (0,1), a second round h2 gives u2 = (h2 >> 8) 2^-24 in [0,1), both exact in fp32.
// cospif takes the exact argument 2 u2, so the error stays relative to |z|; |z| <= sqrt(48 ln 2) = 5.768.
__device__ __forceinline__ float sg_z(unsigned key, unsigned e) {
  const unsigned a = sg_fmix32(key ^ (0x85EBCA77u * (e + 1u)));
  const unsigned h2 = sg_fmix32(a + 0x9E3779B9u);
  const float u1 = (float)(2u * (a >> 9) + 1u) * 0x1p-24f;
  const float u2 = (float)(h2 >> 8) * 0x1p-24f;
  return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

// the sample: the fusion is written out because the library builds with -ffp-contract=off; with sigma == 0 the product
// is a signed zero and p == x
__device__ __forceinline__ float sg_point(float sigma, float z, float xv) { return fmaf(sigma, z, xv); }

constexpr int SG_PIECE = 8;   // frames whose loads a staging thread requests before it starts on their noise

// ---------------------------------------------------------------- explicit noise
__global__ __launch_bounds__(256) void sg_noise_kernel(unsigned seed, int first_k, size_t per_clip, size_t total,
                                                       float* __restrict__ z) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / per_clip);
    z[i] = sg_z(sg_key(seed, first_k + r), (unsigned)(i - (size_t)r * per_clip));
  }
}

// ---------------------------------------------------------------- range
// One workgroup per clip: every thread takes elements tid, tid + 1024, ... (16 bytes at a time where the clip allows
// it), then a wave64 shuffle tree and the 16 waves through LDS.  min and max are exact under any order; fminf / fmaxf
// skip a NaN element.
template <int V>
__global__ __launch_bounds__(1024) void sg_range_kernel(const float* __restrict__ x, size_t per_clip, float level,
                                                        float* __restrict__ sigma) {
  using vec = typename std::conditional<V == 4, float4, float>::type;
  const vec* xc = reinterpret_cast<const vec*>(x + (size_t)blockIdx.x * per_clip);
  const size_t nv = per_clip / V;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  for (size_t i = threadIdx.x; i < nv; i += 1024) {
    const vec v = xc[i];
    if constexpr (V == 4) {
      lo = fminf(fminf(lo, v.x), fminf(v.y, fminf(v.z, v.w)));
      hi = fmaxf(fmaxf(hi, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    } else {
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_down(lo, o, 64));
    hi = fmaxf(hi, __shfl_down(hi, o, 64));
  }
  __shared__ float red[16][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[wave][0] = lo;
    red[wave][1] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; ++w) {
      lo = fminf(lo, red[w][0]);
      hi = fmaxf(hi, red[w][1]);
    }
    sigma[blockIdx.x] = level * (hi - lo);
  }
}

// ---------------------------------------------------------------- stage
// 16-byte channels-last pixels (C <= 4): one thread per (row, pixel), one 16-byte store per frame, pad lanes +0.0; row j
// = sample (first + j) % n of clip (first + j) / n.  The loads of SG_PIECE frames are requested before their noise is
// computed, so the hashes and transcendentals run under the memory time.
__global__ __launch_bounds__(256) void sg_stage_cl4_kernel(const float* __restrict__ x, const float* __restrict__ sigma,
                                                           int C, int T, int HW, int n, unsigned seed, long long first,
                                                           int count, float* __restrict__ p) {
  size_t total = (size_t)count * HW;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int px = i % HW;
    const int j = i / HW;
    const long long g = first + j;
    const int clip = (int)(g / n);
    const unsigned key = sg_key(seed, (int)(g % n));
    const float sg = sigma[clip];
    const float* xc = x + (size_t)clip * C * T * HW + px;
    float* pr = p + ((size_t)j * T * HW + px) * 4;
    for (int u0 = 0; u0 < T; u0 += SG_PIECE) {
      float xv[4][SG_PIECE];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int f = 0; f < SG_PIECE; ++f) {
          xv[c][f] = 0.f;
          if (c < C && u0 + f < T) xv[c][f] = xc[((size_t)c * T + u0 + f) * HW];
        }
#pragma unroll
      for (int f = 0; f < SG_PIECE; ++f) {
        const int u = u0 + f;
        if (u < T) {
          float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (c < C) v[c] = sg_point(sg, sg_z(key, (unsigned)((c * T + u) * HW + px)), xv[c][f]);
          *reinterpret_cast<float4*>(pr + (size_t)u * HW * 4) = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
    }
  }
}

// NCTHW: one thread per (row, channel, 4-pixel quad) when HW % 4 == 0 (16-byte loads and stores), else per pixel
template <int V>
__global__ __launch_bounds__(256) void sg_stage_ncthw_kernel(const float* __restrict__ x, const float* __restrict__ sigma,
                                                             int C, int T, int HW, int n, unsigned seed, long long first,
                                                             int count, float* __restrict__ p) {
  using vec = typename std::conditional<V == 4, float4, float>::type;
  const int HWv = HW / V;
  size_t total = (size_t)count * C * HWv;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int q = i % HWv;
    const int c = (i / HWv) % C;
    const int j = i / ((size_t)HWv * C);
    const long long g = first + j;
    const int clip = (int)(g / n);
    const unsigned key = sg_key(seed, (int)(g % n));
    const float sg = sigma[clip];
    const vec* xc = reinterpret_cast<const vec*>(x + ((size_t)clip * C + c) * T * HW) + q;
    vec* pc = reinterpret_cast<vec*>(p + ((size_t)j * C + c) * T * HW) + q;
    const unsigned e0 = (unsigned)(c * T) * (unsigned)HW + (unsigned)(q * V);
    for (int u0 = 0; u0 < T; u0 += SG_PIECE) {
      vec xv[SG_PIECE];
#pragma unroll
      for (int f = 0; f < SG_PIECE; ++f) {
        xv[f] = vec{};
        if (u0 + f < T) xv[f] = xc[(size_t)(u0 + f) * HWv];
      }
#pragma unroll
      for (int f = 0; f < SG_PIECE; ++f) {
        const int u = u0 + f;
        if (u < T) {
          const unsigned e = e0 + (unsigned)u * (unsigned)HW;
          vec v;
          if constexpr (V == 4) {
            v = make_float4(sg_point(sg, sg_z(key, e), xv[f].x), sg_point(sg, sg_z(key, e + 1), xv[f].y),
                            sg_point(sg, sg_z(key, e + 2), xv[f].z), sg_point(sg, sg_z(key, e + 3), xv[f].w));
          } else {
            v = sg_point(sg, sg_z(key, e), xv[f]);
          }
          pc[(size_t)u * HWv] = v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------- accumulate
// The window holds rows [first, first + count) of the (clip, sample) list, as ig_accumulate_*_kernel: clips c0 =
// first / n .. (first + count - 1) / n.  din is read once for both moments.
// NCTHW: one thread per element (clip, c, t, px) of those clips; it walks the window's rows of its clip in ascending k.
__global__ __launch_bounds__(256) void sg_accumulate_ncthw_kernel(const float* __restrict__ din, int n, long long first,
                                                                  int count, int c0, int nclips, size_t per_clip,
                                                                  float* __restrict__ G1, float* __restrict__ G2) {
  size_t total = (size_t)nclips * per_clip;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i % per_clip;
    const int clip = c0 + (int)(i / per_clip);
    long long lo = (long long)clip * n - first, hi = lo + n;   // rows of this clip, relative to the window
    if (lo < 0) lo = 0;
    if (hi > count) hi = count;
    float a1 = G1[(size_t)clip * per_clip + e], a2 = G2[(size_t)clip * per_clip + e];
    for (long long j = lo; j < hi; ++j) {
      const float g = din[(size_t)j * per_clip + e];
      a1 = a1 + g;
      a2 = fmaf(g, g, a2);
    }
    G1[(size_t)clip * per_clip + e] = a1;
    G2[(size_t)clip * per_clip + e] = a2;
  }
}

// 16-byte channels-last rows [count,T,HW,4]: one thread per pixel (clip, t, px); one 16-byte load per row serves the C
// channels, the pad lanes of din are never read into the arithmetic.
__global__ __launch_bounds__(256) void sg_accumulate_cl4_kernel(const float* __restrict__ din, int n, long long first,
                                                                int count, int c0, int nclips, int C, int T, int HW,
                                                                float* __restrict__ G1, float* __restrict__ G2) {
  const size_t THW = (size_t)T * HW;
  size_t total = (size_t)nclips * THW;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i % THW;
    const int clip = c0 + (int)(i / THW);
    long long lo = (long long)clip * n - first, hi = lo + n;
    if (lo < 0) lo = 0;
    if (hi > count) hi = count;
    float* g1 = G1 + (size_t)clip * C * THW + e;
    float* g2 = G2 + (size_t)clip * C * THW + e;
    float a1[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) {
        a1[c] = g1[(size_t)c * THW];
        a2[c] = g2[(size_t)c * THW];
      }
    for (long long j = lo; j < hi; ++j) {
      const float4 g = *reinterpret_cast<const float4*>(din + ((size_t)j * THW + e) * 4);
      const float gv[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) {
          a1[c] = a1[c] + gv[c];
          a2[c] = fmaf(gv[c], gv[c], a2[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) {
        g1[(size_t)c * THW] = a1[c];
        g2[(size_t)c * THW] = a2[c];
      }
  }
}

// ---------------------------------------------------------------- finish
// One workgroup per (clip, frame), the order of ig_finish_kernel: every thread takes the pixels px = tid, tid + 256, ...
// in that order (the maps are written on the way), then a wave64 shuffle tree, then the four waves in order.  Every
// operation is rounded once in the order written (no contraction), c ascending:
//   m = G1 / n;  sg += |m|;  sq += G2 / n;  var += (G2 - G1 * m) / (n - 1)    (var 0.0 at n == 1)
__global__ __launch_bounds__(256) void sg_finish_kernel(const float* __restrict__ G1, const float* __restrict__ G2, int n,
                                                        int C, int T, int HW, float* __restrict__ sg_map,
                                                        float* __restrict__ sq_map, float* __restrict__ var_map,
                                                        float* __restrict__ sg_frames, float* __restrict__ sq_frames,
                                                        float* __restrict__ var_frames) {
  const int t = blockIdx.x % T, b = blockIdx.x / T;
  const float* g1 = G1 + (size_t)b * C * T * HW;
  const float* g2 = G2 + (size_t)b * C * T * HW;
  const float nf = (float)n, nm1 = (float)(n - 1);
  float v[3] = {0.f, 0.f, 0.f};
  for (int px = threadIdx.x; px < HW; px += 256) {
    float sg = 0.f, sq = 0.f, var = 0.f;
    for (int c = 0; c < C; ++c) {
      const size_t e = ((size_t)c * T + t) * HW + px;
      const float a1 = g1[e], a2 = g2[e];
      const float m = a1 / nf;
      sg += fabsf(m);
      sq += a2 / nf;
      if (n > 1) {
        const float prod = a1 * m;
        const float d = a2 - prod;
        var += d / nm1;
      }
    }
    const size_t o = ((size_t)b * T + t) * HW + px;
    sg_map[o] = sg;
    sq_map[o] = sq;
    var_map[o] = var;
    v[0] += sg;
    v[1] += sq;
    v[2] += var;
  }
  __shared__ float red[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    if (lane == 0) red[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    const float r = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    (k == 0 ? sg_frames : k == 1 ? sq_frames : var_frames)[(size_t)b * T + t] = r;
  }
}

static bool sg_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// C T HW <= 2^31 - 1: the element index and e + 1 fit the hash's 32 bits
static bool sg_dims_ok(int b, int C, int T, int HW) {
  return b > 0 && C > 0 && T > 0 && HW > 0 && (long long)C * T * HW <= 0x7fffffffLL;
}

#define SG_CHECK_DIMS(what, b, C, T, HW) \
  IVF_CHECK_ARG(sg_dims_ok(b, C, T, HW), what ": bad dims (b, C, T, HW > 0 and C T HW <= 2^31 - 1)")
#define SG_CHECK_ROWS(what, first, count, b, n)                                                                       \
  IVF_CHECK_ARG(first >= 0 && count > 0 && first + count <= (long long)b * n,                                           \
                what ": rows [%lld, %lld) outside the %lld samples of %d clips", first, first + count, (long long)b * n, b)
#define SG_CHECK_LAYOUT(what, layout, C)         \
  IVF_CHECK_ARG(layout == 0 || (layout == 4 && C <= 4), what ": layout must be 0 (NCTHW) or 4 (16-byte channels-last, C <= 4)")

}  // namespace ivf

using namespace ivf;

extern "C" size_t ivf_sg_workspace_bytes(int b, int C, int T, int HW, int n) {
  if (!sg_dims_ok(b, C, T, HW) || n <= 0) {
    set_error("sg_workspace_bytes: bad dims");
    return 0;
  }
  return SgScratch().carve((size_t)b, (size_t)C * T * HW, (size_t)n);
}

extern "C" int ivf_sg_noise(unsigned seed, int first_k, int count, int C, int T, int HW, float* z_out,
                            ivf_stream_t stream) {
  IVF_CHECK_ARG(z_out, "sg_noise: null pointer");
  SG_CHECK_DIMS("sg_noise", 1, C, T, HW);
  IVF_CHECK_ARG(first_k >= 0 && count > 0 && (long long)first_k + count <= 0x7fffffffLL,
                "sg_noise: samples [%d, %lld) outside 0 .. 2^31 - 1", first_k, (long long)first_k + count);
  const size_t per_clip = (size_t)C * T * HW, total = per_clip * (size_t)count;
  hipLaunchKernelGGL(sg_noise_kernel, dim3(grid_for(total, 256, 2048)), dim3(256), 0, (hipStream_t)stream, seed, first_k,
                     per_clip, total, z_out);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_sg_range(const float* x, int b, int C, int T, int HW, float level, float* sigma_out,
                            ivf_stream_t stream) {
  IVF_CHECK_ARG(x && sigma_out, "sg_range: null pointer");
  SG_CHECK_DIMS("sg_range", b, C, T, HW);
  IVF_CHECK_ARG(std::isfinite(level) && level >= 0.f, "sg_range: level must be finite and >= 0");
  const size_t per_clip = (size_t)C * T * HW;
  hipStream_t s = (hipStream_t)stream;
  if (per_clip % 4 == 0 && sg_aligned16(x))
    hipLaunchKernelGGL(sg_range_kernel<4>, dim3(b), dim3(1024), 0, s, x, per_clip, level, sigma_out);
  else
    hipLaunchKernelGGL(sg_range_kernel<1>, dim3(b), dim3(1024), 0, s, x, per_clip, level, sigma_out);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_sg_stage(const float* x, const float* sigma, int b, int C, int T, int HW, int n, unsigned seed,
                            long long first, int count, float* out, int layout, ivf_stream_t stream) {
  IVF_CHECK_ARG(x && sigma && out, "sg_stage: null pointer");
  SG_CHECK_DIMS("sg_stage", b, C, T, HW);
  IVF_CHECK_ARG(n > 0, "sg_stage: bad sample count %d", n);
  SG_CHECK_ROWS("sg_stage", first, count, b, n);
  SG_CHECK_LAYOUT("sg_stage", layout, C);
  hipStream_t s = (hipStream_t)stream;
  if (layout == 4) {
    IVF_CHECK_ARG(sg_aligned16(out), "sg_stage: channels-last output must be 16-byte aligned");
    hipLaunchKernelGGL(sg_stage_cl4_kernel, dim3(grid_for((size_t)count * HW, 256, 4096)), dim3(256), 0, s, x, sigma, C, T,
                       HW, n, seed, first, count, out);
  } else if (HW % 4 == 0 && sg_aligned16(x) && sg_aligned16(out)) {
    hipLaunchKernelGGL(sg_stage_ncthw_kernel<4>, dim3(grid_for((size_t)count * C * HW / 4, 256, 4096)), dim3(256), 0, s, x,
                       sigma, C, T, HW, n, seed, first, count, out);
  } else {
    hipLaunchKernelGGL(sg_stage_ncthw_kernel<1>, dim3(grid_for((size_t)count * C * HW, 256, 4096)), dim3(256), 0, s, x,
                       sigma, C, T, HW, n, seed, first, count, out);
  }
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_sg_accumulate(const float* din, int layout, int n, long long first, int count, float* G1, float* G2,
                                 int b, int C, int T, int HW, ivf_stream_t stream) {
  IVF_CHECK_ARG(din && G1 && G2, "sg_accumulate: null pointer");
  SG_CHECK_DIMS("sg_accumulate", b, C, T, HW);
  IVF_CHECK_ARG(n > 0, "sg_accumulate: bad sample count %d", n);
  SG_CHECK_ROWS("sg_accumulate", first, count, b, n);
  SG_CHECK_LAYOUT("sg_accumulate", layout, C);
  const int c0 = (int)(first / n), nclips = (int)((first + count - 1) / n) - c0 + 1;
  hipStream_t s = (hipStream_t)stream;
  if (layout == 4) {
    IVF_CHECK_ARG(sg_aligned16(din), "sg_accumulate: channels-last gradient must be 16-byte aligned");
    hipLaunchKernelGGL(sg_accumulate_cl4_kernel, dim3(grid_for((size_t)nclips * T * HW, 256, 4096)), dim3(256), 0, s, din, n,
                       first, count, c0, nclips, C, T, HW, G1, G2);
  } else {
    const size_t per_clip = (size_t)C * T * HW;
    hipLaunchKernelGGL(sg_accumulate_ncthw_kernel, dim3(grid_for((size_t)nclips * per_clip, 256, 4096)), dim3(256), 0, s,
                       din, n, first, count, c0, nclips, per_clip, G1, G2);
  }
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_sg_finish(const float* G1, const float* G2, int n, int b, int C, int T, int HW, float* sg_map,
                             float* sq_map, float* var_map, float* sg_frames, float* sq_frames, float* var_frames,
                             ivf_stream_t stream) {
  IVF_CHECK_ARG(G1 && G2 && sg_map && sq_map && var_map && sg_frames && sq_frames && var_frames, "sg_finish: null pointer");
  SG_CHECK_DIMS("sg_finish", b, C, T, HW);
  IVF_CHECK_ARG((long long)b * T <= 0x7fffffffLL, "sg_finish: too many frames");
  IVF_CHECK_ARG(n > 0 && n <= (1 << 24), "sg_finish: sample count %d outside 1 .. 2^24", n);
  hipLaunchKernelGGL(sg_finish_kernel, dim3(b * T), dim3(256), 0, (hipStream_t)stream, G1, G2, n, C, T, HW, sg_map, sq_map,
                     var_map, sg_frames, sq_frames, var_frames);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}
