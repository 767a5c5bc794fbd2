// Shapley value sampling for video (Castro et al. 2009; Strumbelj & Kononenko 2014), an EXTENSION with no counterpart
// in the reference.  The players are the cells of a grid (gt, gh, gw), a coalition is the set of frozen
// cells, its value the class score of the clip frozen per pixel by that binary mask.  Permutation sampling: along
// permutation k the cells are frozen one after another, prefix j = the j cells of lowest rank frozen, and the marginal
// of cell c is the score drop on its entry,
//   d_k[c] = s[k][rank_k[c]] - s[k][rank_k[c] + 1],         phi[c] = mean_k d_k[c]     (phi > 0: freezing c lowers the score)
// so that sum_c d_k[c] = s[k][0] - s[k][P] telescopes for every k: the clip's score minus the fully frozen clip's.
//
// The permutation family is integer-exact and the same for every clip.  With the hash of the RISE masks (restated here
// so that rise_ops.hip stays as it is),
//   h(seed, k, c) = fmix32( fmix32(seed + 0x9E3779B9 (k + 1)) ^ (0x85EBCA77 (c + 1)) )                (uint32, wrapping)
//   rank_k[c] = #{c' : (h(seed,k,c'), c') < (h(seed,k,c), c)}                        (lexicographic: a tie falls to the lower index)
// and, antithetic, an odd k is permutation k - 1 (hashed as itself) reversed: rank_k[c] = P - 1 - rank_{k-1}[c].
//
// Staging writes what ivf_stmask_expand_fwd + ivf_stfreeze_fwd write for the row's explicit S [T,gh,gw] (S[u][c] = 1 iff
// rank_k[c] < j in the temporal cell of frame u), without S or M in memory: with S in {0, 1} the expand's sums lose their
// zero terms exactly (the comment above box_mask_at in stmask_ops.hip), so per pixel and temporal cell
//   tmp[i] = sum_{j set, ascending} A_W[x,j]
//   M      = sum_{i ascending, all i} A_H[y,i] * tmp[i]
// every partial sum rounded as stmask_expand_fwd_kernel rounds it, then the recurrence expression of ivf_stfreeze_fwd.
// The scan is the one of rise_ops.hip; only the source of the column words differs (a rank table, not a threshold).
#include "search_driver.h"

namespace ivf {

constexpr int SHAP_MAX_GRID = 32;      // gh, gw: the bits of a grid row are one 32-bit word
constexpr int SHAP_MAX_PLAYERS = 4096; // ranks fit in uint16, a permutation's hashes in 16 KiB of LDS

struct ShapGrid {
  int gt, gh, gw, n;     // n: permutations per clip; a clip has n (P + 1) rows
};

__device__ __forceinline__ unsigned shap_fmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
__device__ __forceinline__ unsigned shap_key(unsigned seed, int k) { return shap_fmix32(seed + 0x9E3779B9u * (unsigned)(k + 1)); }
__device__ __forceinline__ unsigned shap_hash(unsigned key, int c) { return shap_fmix32(key ^ (0x85EBCA77u * (unsigned)(c + 1))); }

// ---------------------------------------------------------------- rank table
// One workgroup per permutation: the P hashes go to LDS once, then every thread counts, for its cells, the hashes below
// its own (all lanes read the same LDS word: a broadcast, no bank conflict).  A counting rank, not a sort: it needs one
// barrier, gives the rank (the inverse permutation a sort would still have to scatter) directly, and breaks ties by
// index for free.  At P = 4096 that is 2^24 compares per permutation, 65,536 per thread: 1.6 ms for 64 permutations
// (measured), once per call, beside n (P + 1) forward passes.
__global__ __launch_bounds__(256) void shap_ranks_kernel(unsigned seed, int antithetic, int first_k, int P,
                                                         unsigned short* __restrict__ ranks) {
  __shared__ unsigned hs[SHAP_MAX_PLAYERS];
  const int k = first_k + blockIdx.x;
  const bool rev = antithetic && (k & 1);
  const unsigned key = shap_key(seed, rev ? k - 1 : k);
  for (int c = threadIdx.x; c < P; c += 256) hs[c] = shap_hash(key, c);
  __syncthreads();
  unsigned short* out = ranks + (size_t)blockIdx.x * P;
  for (int c = threadIdx.x; c < P; c += 256) {
    const unsigned h = hs[c];
    int r = 0;
    for (int o = 0; o < P; ++o) {
      const unsigned v = hs[o];
      r += (v < h || (v == h && o < c)) ? 1 : 0;
    }
    out[c] = (unsigned short)(rev ? P - 1 - r : r);
  }
}

// ---------------------------------------------------------------- staging
// One workgroup per (row, 256 pixels), as rise_stage: the row's gt * gh column words (bit jj = cell (kt, i, jj) frozen =
// its rank below the row's prefix length) are built once in LDS from the rank table; every thread parks row x of A_W in
// its own LDS column.  The words are the workgroup's, so the loop over the set bits is uniform.
struct ShapLds {
  unsigned* word;
  float* aw;
};

__device__ __forceinline__ ShapLds shap_fill_lds(unsigned* lds, const float* __restrict__ AW,
                                                 const unsigned short* __restrict__ rk, const ShapGrid& g, int prefix,
                                                 int x) {
  ShapLds l;
  l.word = lds;
  l.aw = reinterpret_cast<float*>(lds + g.gt * g.gh);
  const int tid = threadIdx.x;
  for (int w = tid; w < g.gt * g.gh; w += 256) {
    unsigned bits = 0;
    for (int j = 0; j < g.gw; ++j) bits |= ((int)rk[w * g.gw + j] < prefix ? 1u : 0u) << j;
    l.word[w] = bits;
  }
  for (int j = 0; j < g.gw; ++j) l.aw[j * 256 + tid] = AW[(size_t)x * g.gw + j];
  __syncthreads();
  return l;
}

__device__ __forceinline__ float shap_mask_at(const ShapLds& l, const float* __restrict__ AHy, int gh, int kt) {
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

// row r of the flattened (clip, permutation, prefix) list
struct ShapRow {
  int clip, k, prefix;
};
__device__ __forceinline__ ShapRow shap_row(long long r, int n, int P) {
  const long long per = (long long)n * (P + 1);
  const int in_clip = (int)(r % per);
  return {(int)(r / per), in_clip / (P + 1), in_clip % (P + 1)};
}

// 16-byte channels-last pixels (C <= 4), as rise_stage_cl4_kernel: with TT > 0 (T == TT) the 16 frames of a piece are
// requested before the scan goes over them.
template <int TT>   // 0, or a multiple of 16
__global__ __launch_bounds__(256) void shap_stage_cl4_kernel(const float* __restrict__ x, const float* __restrict__ AH,
                                                             const float* __restrict__ AW,
                                                             const unsigned short* __restrict__ ranks,
                                                             float* __restrict__ p, int C, int Trun, int W, int HW,
                                                             ShapGrid g, long long first) {
  extern __shared__ unsigned shap_lds[];
  const int row = blockIdx.y, T = TT > 0 ? TT : Trun, P = g.gt * g.gh * g.gw;
  const ShapRow q = shap_row(first + row, g.n, P);
  const int pxu = blockIdx.x * 256 + threadIdx.x;
  const int px = min(pxu, HW - 1);          // threads past the end stage LDS for a valid pixel, then leave
  const ShapLds l = shap_fill_lds(shap_lds, AW, ranks + (size_t)q.k * P, g, q.prefix, px % W);
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
        if (kt != cur) {
          cur = kt;
          m = shap_mask_at(l, AHy, g.gh, kt);
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
        m = shap_mask_at(l, AHy, g.gh, kt);
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
__global__ __launch_bounds__(256) void shap_stage_ncthw_kernel(const float* __restrict__ x, const float* __restrict__ AH,
                                                               const float* __restrict__ AW,
                                                               const unsigned short* __restrict__ ranks,
                                                               float* __restrict__ p, int C, int T, int W, int HW,
                                                               ShapGrid g, long long first) {
  extern __shared__ unsigned shap_lds[];
  const int row = blockIdx.y, P = g.gt * g.gh * g.gw;
  const ShapRow q = shap_row(first + row, g.n, P);
  const int pxu = blockIdx.x * 256 + threadIdx.x;
  const int px = min(pxu, HW - 1);
  const ShapLds l = shap_fill_lds(shap_lds, AW, ranks + (size_t)q.k * P, g, q.prefix, px % W);
  if (pxu >= HW) return;
  const float* AHy = AH + (size_t)(px / W) * g.gh;
  for (int ch = 0; ch < C; ++ch) {
    const float* xp = x + ((size_t)q.clip * C + ch) * T * HW + px;
    float* pp = p + ((size_t)row * C + ch) * T * HW + px;
    float prev = 0.f, m = 0.f;
    int cur = -1;
    for (int u = 0; u < T; ++u) {
      const int kt = (u * g.gt) / T;
      if (kt != cur) {
        cur = kt;
        m = shap_mask_at(l, AHy, g.gh, kt);
      }
      float xv = xp[(size_t)u * HW];
      float v = u ? (1.f - m) * xv + m * prev : xv;
      prev = v;
      pp[(size_t)u * HW] = v;
    }
  }
}

// ---------------------------------------------------------------- reduction
// One thread per (clip, cell) walks the permutations in ascending k twice: the mean of the marginals it can form (a
// term with a NaN score on either side is neither summed nor counted), then the squared deviations from that mean.
// Plain fp32 in a fixed order, no atomics: a clip's numbers do not depend on the batch.  A rank outside [0, P) -- the
// table is the caller's -- forms no term (it would read beyond the permutation's scores).  The thread of a clip's cell
// 0 also walks the end scores of every permutation for `total`.
__global__ __launch_bounds__(256) void shap_reduce_kernel(const float* __restrict__ scores,
                                                          const unsigned short* __restrict__ ranks, int B, int n, int P,
                                                          float* __restrict__ cells_out, float* __restrict__ stderr_out,
                                                          int* __restrict__ count_out, float* __restrict__ total) {
  const size_t e = blockIdx.x * (size_t)256 + threadIdx.x;
  if (e >= (size_t)B * P) return;
  const int b = (int)(e / P), c = (int)(e - (size_t)b * P);
  const float* s = scores + (size_t)b * n * (P + 1);
  const float nan = __builtin_nanf("");
  float sum = 0.f;
  int cnt = 0;
  for (int k = 0; k < n; ++k) {
    const int r = ranks[(size_t)k * P + c];
    if (r >= P) continue;
    const float a = s[(size_t)k * (P + 1) + r], z = s[(size_t)k * (P + 1) + r + 1];
    if (a != a || z != z) continue;
    sum += a - z;
    ++cnt;
  }
  const float mean = cnt ? sum / (float)cnt : nan;
  float ss = 0.f;
  if (cnt >= 2)
    for (int k = 0; k < n; ++k) {
      const int r = ranks[(size_t)k * P + c];
      if (r >= P) continue;
      const float a = s[(size_t)k * (P + 1) + r], z = s[(size_t)k * (P + 1) + r + 1];
      if (a != a || z != z) continue;
      const float dev = (a - z) - mean;
      ss += dev * dev;
    }
  cells_out[e] = mean;
  stderr_out[e] = cnt >= 2 ? sqrtf(ss / (float)(cnt - 1) / (float)cnt) : nan;
  count_out[e] = cnt;
  if (c == 0) {
    float all = 0.f;
    int nall = 0;
    for (int k = 0; k < n; ++k) {
      const float a = s[(size_t)k * (P + 1)], z = s[(size_t)k * (P + 1) + P];
      if (!(__builtin_isfinite(a) && __builtin_isfinite(z))) continue;
      all += a - z;
      ++nall;
    }
    total[b] = nall ? all / (float)nall : nan;
  }
}

static bool shap_grid_ok(int T, int gt, int gh, int gw) {
  return T >= 1 && T <= MAX_T && gt >= 1 && gt <= T && gh >= 1 && gh <= SHAP_MAX_GRID && gw >= 1 && gw <= SHAP_MAX_GRID &&
         gt * gh * gw <= SHAP_MAX_PLAYERS;
}

#define SHAP_CHECK_GRID(what, T, gt, gh, gw)                                                                             \
  IVF_CHECK_ARG(shap_grid_ok(T, gt, gh, gw),                                                                             \
                what ": need 1 <= gt (%d) <= T (%d) <= %d, 1 <= gh (%d), gw (%d) <= %d and gt gh gw <= %d players", gt, T, \
                MAX_T, gh, gw, SHAP_MAX_GRID, SHAP_MAX_PLAYERS)

}  // namespace ivf

using namespace ivf;

extern "C" int ivf_shap_ranks(unsigned seed, int antithetic, int first_k, int count, int gt, int gh, int gw,
                              unsigned short* ranks, ivf_stream_t stream) {
  IVF_CHECK_ARG(ranks, "shap_ranks: null pointer");
  SHAP_CHECK_GRID("shap_ranks", MAX_T, gt, gh, gw);     // the clip length is not this entry's: gt <= MAX_T
  IVF_CHECK_ARG(antithetic == 0 || antithetic == 1, "shap_ranks: antithetic must be 0 or 1, got %d", antithetic);
  IVF_CHECK_ARG(first_k >= 0 && count > 0 && (long long)first_k + count <= 0x7fffffffLL,
                "shap_ranks: permutations [%d, %lld) outside 0 .. 2^31 - 1", first_k, (long long)first_k + count);
  hipLaunchKernelGGL(shap_ranks_kernel, dim3(count), dim3(256), 0, (hipStream_t)stream, seed, antithetic, first_k,
                     gt * gh * gw, ranks);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_shap_stage(const float* x, int b, int C, int T, int H, int W, const float* A_H, const float* A_W, int gt,
                              int gh, int gw, int n, const unsigned short* ranks, long long first, int count, float* p,
                              int out_cpad, ivf_stream_t stream) {
  IVF_CHECK_ARG(x && A_H && A_W && ranks && p, "shap_stage: null pointer");
  IVF_CHECK_ARG(b > 0 && C > 0 && H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL, "shap_stage: bad dims");
  SHAP_CHECK_GRID("shap_stage", T, gt, gh, gw);
  IVF_CHECK_ARG(n > 0 && (long long)n * (gt * gh * gw + 1) <= 0x7fffffffLL, "shap_stage: bad permutation count %d", n);
  const long long rows = (long long)b * n * (gt * gh * gw + 1);
  IVF_CHECK_ARG(first >= 0 && count > 0 && count <= 65535 && first + count <= rows,
                "shap_stage: rows [%lld, %lld) outside the %lld rows of %d clips (at most 65535 rows a call)", first,
                first + count, rows, b);
  IVF_CHECK_ARG(out_cpad == 0 || (out_cpad == 4 && C <= 4),
                "shap_stage: out_cpad must be 0 (NCTHW) or 4 (16-byte channels-last, C <= 4)");
  IVF_CHECK_ARG(out_cpad == 0 || ((uintptr_t)p & 15) == 0, "shap_stage: the channels-last buffer is not 16-byte aligned");
  const ShapGrid g{gt, gh, gw, n};
  const int HW = H * W;
  const size_t lds = ((size_t)gt * gh + (size_t)gw * 256) * 4;      // at most 8 + 32 KiB
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(cdiv(HW, 256), count), block(256);
  if (out_cpad == 0)
    hipLaunchKernelGGL(shap_stage_ncthw_kernel, grid, block, lds, s, x, A_H, A_W, ranks, p, C, T, W, HW, g, first);
  else
    with_frames_exact(T, [&](auto TT) {
      hipLaunchKernelGGL(shap_stage_cl4_kernel<TT>, grid, block, lds, s, x, A_H, A_W, ranks, p, C, T, W, HW, g, first);
    });
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_shap_reduce(const float* scores, const unsigned short* ranks, int b, int n, int gt, int gh, int gw,
                               float* cells, float* stderr_out, int* count, float* total, ivf_stream_t stream) {
  IVF_CHECK_ARG(scores && ranks && cells && stderr_out && count && total, "shap_reduce: null pointer");
  IVF_CHECK_ARG(b > 0 && n > 0, "shap_reduce: bad batch %d or permutation count %d", b, n);
  SHAP_CHECK_GRID("shap_reduce", MAX_T, gt, gh, gw);
  const int P = gt * gh * gw;
  const long long all = (long long)b * P;
  IVF_CHECK_ARG((all + 255) / 256 <= 0x7fffffffLL, "shap_reduce: too many cells");
  hipLaunchKernelGGL(shap_reduce_kernel, dim3(cdiv(all, 256)), dim3(256), 0, (hipStream_t)stream, scores, ranks, b, n, P,
                     cells, stderr_out, count, total);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}
