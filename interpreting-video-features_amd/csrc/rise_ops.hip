// RISE random-mask saliency for video (Petsiuk et al. 2018), an EXTENSION with no counterpart in the reference
// (DESIGN 14): n random coarse masks per clip, one forward each, a cell's importance = the mean score drop over the
// masks that froze it.
//
// The mask family is integer-exact and the same for every clip.  A mask lives on a grid (gt, gh, gw); frame u belongs
// to temporal cell kt = (u gt) / T, cell c = (kt gh + i) gw + j, and mask k freezes cell c iff
//   u(seed, k, c) = fmix32( fmix32(seed + 0x9E3779B9 (k + 1)) ^ (0x85EBCA77 (c + 1)) ) < thresh        (uint32, wrapping)
// with fmix32 the finaliser of MurmurHash3.  Nothing stores the masks: staging and reduction regenerate the bits.
//
// Staging writes what ivf_stmask_expand_fwd + ivf_stfreeze_fwd write for the row's explicit S [T,gh,gw] (S[u] =
// S_k[kt(u)]), without S or M in memory.  With S in {0, 1} the expand's sums lose their zero terms exactly (the comment
// above box_mask_at in stmask_ops.hip), so per pixel and temporal cell
//   tmp[i] = sum_{j set, ascending} A_W[x,j]
//   M      = sum_{i ascending, all i} A_H[y,i] * tmp[i]
// every partial sum rounded as stmask_expand_fwd_kernel rounds it (no contraction: a multiply and an add each), then the
// recurrence expression of ivf_stfreeze_fwd.
#include "search_driver.h"

namespace ivf {

constexpr int RISE_MAX_GRID = 32;   // gh, gw: the bits of a grid row are one 32-bit word

struct RiseGrid {
  int gt, gh, gw, n;
  unsigned seed, thresh;
};

__device__ __forceinline__ unsigned rise_fmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
// the part of u(seed, k, c) that belongs to the mask, and the rest
__device__ __forceinline__ unsigned rise_key(unsigned seed, int k) { return rise_fmix32(seed + 0x9E3779B9u * (unsigned)(k + 1)); }
__device__ __forceinline__ bool rise_bit(unsigned key, int c, unsigned thresh) {
  return rise_fmix32(key ^ (0x85EBCA77u * (unsigned)(c + 1))) < thresh;
}

// ---------------------------------------------------------------- explicit bits
__global__ __launch_bounds__(256) void rise_masks_kernel(RiseGrid g, int first_k, int count, float* __restrict__ S) {
  const int cells = g.gt * g.gh * g.gw;
  const size_t e = blockIdx.x * (size_t)256 + threadIdx.x;
  if (e >= (size_t)count * cells) return;
  const int r = (int)(e / cells), c = (int)(e - (size_t)r * cells);
  S[e] = rise_bit(rise_key(g.seed, first_k + r), c, g.thresh) ? 1.f : 0.f;
}

// ---------------------------------------------------------------- staging
// One workgroup per (row, 256 pixels).  The row's gt * gh column words (bit j = cell (kt, i, j) frozen) are hashed once
// into LDS; every thread parks row x of A_W in its own LDS column (aw_s[j * 256 + tid]: a wave reads 64 consecutive
// words, no bank conflict, and nobody reads another thread's column).  The words are the workgroup's, so the loop over
// the set bits is uniform.  M is computed once on entering a temporal cell.
struct RiseLds {
  unsigned* word;
  float* aw;
};

__device__ __forceinline__ RiseLds rise_fill_lds(unsigned* lds, const float* __restrict__ AW, const RiseGrid& g, int k,
                                                 int x) {
  RiseLds l;
  l.word = lds;
  l.aw = reinterpret_cast<float*>(lds + g.gt * g.gh);
  const int tid = threadIdx.x;
  const unsigned key = rise_key(g.seed, k);
  for (int w = tid; w < g.gt * g.gh; w += 256) {
    unsigned bits = 0;
    for (int j = 0; j < g.gw; ++j) bits |= (rise_bit(key, w * g.gw + j, g.thresh) ? 1u : 0u) << j;
    l.word[w] = bits;
  }
  for (int j = 0; j < g.gw; ++j) l.aw[j * 256 + tid] = AW[(size_t)x * g.gw + j];
  __syncthreads();
  return l;
}

// M[y,x] of the row's mask on the frames of temporal cell kt; A_H row y is read through the cache (a wave mostly
// shares its row y)
__device__ __forceinline__ float rise_mask_at(const RiseLds& l, const float* __restrict__ AHy, int gh, int kt) {
  float m = 0.f;
  for (int i = 0; i < gh; ++i) {
    unsigned w = l.word[kt * gh + i];
    float t = 0.f;
    while (w) {
      t += l.aw[(__ffs(w) - 1) * 256 + threadIdx.x];
      w &= w - 1;
    }
    m += AHy[i] * t;
  }
  return m;
}

// 16-byte channels-last pixels (C <= 4), as box_stage_cl4_kernel: with TT > 0 (T == TT) the 16 frames of a piece are
// requested before the scan goes over them.
template <int TT>   // 0, or a multiple of 16
__global__ __launch_bounds__(256) void rise_stage_cl4_kernel(const float* __restrict__ x, const float* __restrict__ AH,
                                                             const float* __restrict__ AW, float* __restrict__ p, int C,
                                                             int Trun, int W, int HW, RiseGrid g, long long first) {
  extern __shared__ unsigned rise_lds[];
  const int row = blockIdx.y, T = TT > 0 ? TT : Trun;
  const long long r = first + row;
  const int clip = (int)(r / g.n), k = (int)(r % g.n);
  const int pxu = blockIdx.x * 256 + threadIdx.x;
  const int px = min(pxu, HW - 1);          // threads past the end stage LDS for a valid pixel, then leave
  const RiseLds l = rise_fill_lds(rise_lds, AW, g, k, px % W);
  if (pxu >= HW) return;
  const float* AHy = AH + (size_t)(px / W) * g.gh;
  const float* xc = x + (size_t)clip * C * T * HW + px;
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
        if (kt != cur) {
          cur = kt;
          m = rise_mask_at(l, AHy, g.gh, kt);
        }
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
          if (ch < C) {
            v[ch] = u ? (1.f - m) * xv[ch][j] + m * prev[ch] : xv[ch][j];
            prev[ch] = v[ch];
          }
        *reinterpret_cast<float4*>(pr + (size_t)u * HW * 4) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  } else {
    for (int u = 0; u < T; ++u) {
      const int kt = (u * g.gt) / T;
      if (kt != cur) {
        cur = kt;
        m = rise_mask_at(l, AHy, g.gh, kt);
      }
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      for (int ch = 0; ch < C; ++ch) {
        float xv = xc[((size_t)ch * T + u) * HW];
        v[ch] = u ? (1.f - m) * xv + m * prev[ch] : xv;
        prev[ch] = v[ch];
      }
      *reinterpret_cast<float4*>(pr + (size_t)u * HW * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// NCTHW: channel after channel (the mask value is the pixel's, not the channel's; it is recomputed per channel from LDS)
__global__ __launch_bounds__(256) void rise_stage_ncthw_kernel(const float* __restrict__ x, const float* __restrict__ AH,
                                                               const float* __restrict__ AW, float* __restrict__ p, int C,
                                                               int T, int W, int HW, RiseGrid g, long long first) {
  extern __shared__ unsigned rise_lds[];
  const int row = blockIdx.y;
  const long long r = first + row;
  const int clip = (int)(r / g.n), k = (int)(r % g.n);
  const int pxu = blockIdx.x * 256 + threadIdx.x;
  const int px = min(pxu, HW - 1);
  const RiseLds l = rise_fill_lds(rise_lds, AW, g, k, px % W);
  if (pxu >= HW) return;
  const float* AHy = AH + (size_t)(px / W) * g.gh;
  for (int ch = 0; ch < C; ++ch) {
    const float* xp = x + ((size_t)clip * C + ch) * T * HW + px;
    float* pp = p + ((size_t)row * C + ch) * T * HW + px;
    float prev = 0.f, m = 0.f;
    int cur = -1;
    for (int u = 0; u < T; ++u) {
      const int kt = (u * g.gt) / T;
      if (kt != cur) {
        cur = kt;
        m = rise_mask_at(l, AHy, g.gh, kt);
      }
      float xv = xp[(size_t)u * HW];
      float v = u ? (1.f - m) * xv + m * prev : xv;
      prev = v;
      pp[(size_t)u * HW] = v;
    }
  }
}

// ---------------------------------------------------------------- reduction
// One thread per (clip, cell) walks the masks in ascending k, d_k = orig - s_k: cells = sum over the masks that froze
// the cell / their count, a NaN score neither summed nor counted (as ivf_box_drop), NaN where nothing is counted.  The
// thread of a clip's cell 0 also walks all of the clip's masks for mean_drop.  Plain fp32 adds in a fixed order, no
// atomics, the bits regenerated from the hash: a clip's numbers do not depend on the batch.
__global__ __launch_bounds__(256) void rise_reduce_kernel(const float* __restrict__ scores, const float* __restrict__ orig,
                                                          int B, RiseGrid g, float* __restrict__ cells_out,
                                                          int* __restrict__ count_out, float* __restrict__ mean_drop) {
  const int cells = g.gt * g.gh * g.gw;
  const size_t e = blockIdx.x * (size_t)256 + threadIdx.x;
  if (e >= (size_t)B * cells) return;
  const int b = (int)(e / cells), c = (int)(e - (size_t)b * cells);
  const float* s = scores + (size_t)b * g.n;
  const float o = orig[b];
  float sum = 0.f, all = 0.f;
  int cnt = 0, nall = 0;
  for (int k = 0; k < g.n; ++k) {
    const float v = s[k];
    if (v != v) continue;
    const float d = o - v;
    all += d;
    ++nall;
    if (rise_bit(rise_key(g.seed, k), c, g.thresh)) {
      sum += d;
      ++cnt;
    }
  }
  cells_out[e] = cnt ? sum / (float)cnt : __builtin_nanf("");
  count_out[e] = cnt;
  if (c == 0) mean_drop[b] = nall ? all / (float)nall : __builtin_nanf("");
}

static bool rise_grid_ok(int T, int gt, int gh, int gw) {
  return T >= 1 && T <= MAX_T && gt >= 1 && gt <= T && gh >= 1 && gh <= RISE_MAX_GRID && gw >= 1 && gw <= RISE_MAX_GRID;
}

#define RISE_CHECK_GRID(what, T, gt, gh, gw)                                                                            \
  IVF_CHECK_ARG(rise_grid_ok(T, gt, gh, gw), what ": need 1 <= gt (%d) <= T (%d) <= %d and 1 <= gh (%d), gw (%d) <= %d", \
                gt, T, MAX_T, gh, gw, RISE_MAX_GRID)

}  // namespace ivf

using namespace ivf;

extern "C" int ivf_rise_masks(unsigned seed, unsigned thresh, int first_k, int count, int gt, int gh, int gw, float* S,
                              ivf_stream_t stream) {
  IVF_CHECK_ARG(S, "rise_masks: null pointer");
  RISE_CHECK_GRID("rise_masks", MAX_T, gt, gh, gw);     // the clip length is not this entry's: gt <= MAX_T
  IVF_CHECK_ARG(thresh != 0, "rise_masks: thresh must be > 0 (thresh = floor(p 2^32), 0 < p < 1)");
  IVF_CHECK_ARG(first_k >= 0 && count > 0 && (long long)first_k + count <= 0x7fffffffLL,
                "rise_masks: masks [%d, %lld) outside 0 .. 2^31 - 1", first_k, (long long)first_k + count);
  const long long total = (long long)count * gt * gh * gw;
  IVF_CHECK_ARG((total + 255) / 256 <= 0x7fffffffLL, "rise_masks: too many cells");
  const RiseGrid g{gt, gh, gw, 0, seed, thresh};
  hipLaunchKernelGGL(rise_masks_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, g, first_k, count, S);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_rise_stage(const float* x, int b, int C, int T, int H, int W, const float* A_H, const float* A_W, int gt,
                              int gh, int gw, int n, unsigned seed, unsigned thresh, long long first, int count, float* p,
                              int out_cpad, ivf_stream_t stream) {
  IVF_CHECK_ARG(x && A_H && A_W && p, "rise_stage: null pointer");
  IVF_CHECK_ARG(b > 0 && C > 0 && H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL, "rise_stage: bad dims");
  RISE_CHECK_GRID("rise_stage", T, gt, gh, gw);
  IVF_CHECK_ARG(thresh != 0, "rise_stage: thresh must be > 0 (thresh = floor(p 2^32), 0 < p < 1)");
  IVF_CHECK_ARG(n > 0, "rise_stage: bad mask count %d", n);
  IVF_CHECK_ARG(first >= 0 && count > 0 && count <= 65535 && first + count <= (long long)b * n,
                "rise_stage: rows [%lld, %lld) outside the %lld masks of %d clips (at most 65535 rows a call)", first,
                first + count, (long long)b * n, b);
  IVF_CHECK_ARG(out_cpad == 0 || (out_cpad == 4 && C <= 4),
                "rise_stage: out_cpad must be 0 (NCTHW) or 4 (16-byte channels-last, C <= 4)");
  IVF_CHECK_ARG(out_cpad == 0 || ((uintptr_t)p & 15) == 0, "rise_stage: the channels-last buffer is not 16-byte aligned");
  const RiseGrid g{gt, gh, gw, n, seed, thresh};
  const int HW = H * W;
  const size_t lds = ((size_t)gt * gh + (size_t)gw * 256) * 4;      // at most 8 + 32 KiB
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(cdiv(HW, 256), count), block(256);
  if (out_cpad == 0)
    hipLaunchKernelGGL(rise_stage_ncthw_kernel, grid, block, lds, s, x, A_H, A_W, p, C, T, W, HW, g, first);
  else
    with_frames_exact(T, [&](auto TT) {
      hipLaunchKernelGGL(rise_stage_cl4_kernel<TT>, grid, block, lds, s, x, A_H, A_W, p, C, T, W, HW, g, first);
    });
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_rise_reduce(const float* scores, const float* orig, int b, int n, unsigned seed, unsigned thresh, int gt,
                               int gh, int gw, float* cells, int* count, float* mean_drop, ivf_stream_t stream) {
  IVF_CHECK_ARG(scores && orig && cells && count && mean_drop, "rise_reduce: null pointer");
  IVF_CHECK_ARG(b > 0 && n > 0, "rise_reduce: bad batch %d or mask count %d", b, n);
  RISE_CHECK_GRID("rise_reduce", MAX_T, gt, gh, gw);
  IVF_CHECK_ARG(thresh != 0, "rise_reduce: thresh must be > 0 (thresh = floor(p 2^32), 0 < p < 1)");
  const long long total = (long long)b * gt * gh * gw;
  IVF_CHECK_ARG((total + 255) / 256 <= 0x7fffffffLL, "rise_reduce: too many cells");
  const RiseGrid g{gt, gh, gw, n, seed, thresh};
  hipLaunchKernelGGL(rise_reduce_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, scores, orig, b, g,
                     cells, count, mean_drop);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}
