// Deletion / insertion curves (Petsiuk et al. 2018), an EXTENSION with no counterpart in the reference: the
// faithfulness measure that compares the attribution methods.  The players are the cells of a grid (gt, gh, gw) as in
// shapley_ops.hip; an attribution ranks them (a higher value = more important), and the curve is the class score while
// the cells are frozen (deletion) or released (insertion) in that order, `step` cells per row:
//   J = ceil(P / step),   k_j = min(j step, P),   j = 0 .. J
//   deletion row j : cell c frozen iff rank[c] <  k_j        (row 0 the clip, row J the fully frozen clip)
//   insertion row j: cell c frozen iff rank[c] >= k_j        (row 0 the fully frozen clip, row J the clip)
// A deletion curve at step 1 is one Shapley permutation whose rank table comes from the attribution, not from the hash.
//
// Rank (per clip, on the device).  order 0, most relevant first:
//   rank[c] = #{c' : a[c'] > a[c], or a[c'] == a[c] and c' < c}
// order 1 flips > to <.  A NaN cell ranks after every number in either order, the NaN cells among themselves by index;
// -0.0 == +0.0 is a tie.  Every row is a permutation of 0 .. P-1.
//
// Staging writes what ivf_stmask_expand_fwd + ivf_stfreeze_fwd write for the row's explicit binary S, neither S nor M in
// memory; the scan is the one of shapley_ops.hip (restated here so that file stays as it is), only the column words
// differ: a per-clip table, a threshold of several cells, and the insertion test.  Rows are flattened as
// [clip][curve][j], so a chunk of the plan's batch crosses clip and curve boundaries.
//
// Reduction.  auc = (1 / (2P)) sum_{j<J} (k_{j+1} - k_j) (s_j + s_{j+1}): the trapezoid over the fraction of cells.
#include "search_driver.h"

namespace ivf {

constexpr int CURVE_MAX_GRID = 32;      // gh, gw: the bits of a grid row are one 32-bit word
constexpr int CURVE_MAX_PLAYERS = 4096; // ranks fit in uint16, a clip's keys in 16 KiB of LDS

struct CurveGrid {
  int gt, gh, gw;
  int curves, ncurves;   // bit 0 deletion, bit 1 insertion; ncurves = their number
  int step, J;           // a clip has ncurves (J + 1) rows
};

// ---------------------------------------------------------------- rank table
// An unsigned key whose ascending order is the rank order: the usual monotone map of the float's bits (negative: all
// bits flipped; else the sign bit set), -0.0 first made +0.0, complemented for order 0 (descending), and every NaN the
// one key above all others (~(+inf) and +inf both stay below 0xFFFFFFFF).
__device__ __forceinline__ unsigned curve_key(float a, int order) {
  if (a != a) return 0xFFFFFFFFu;
  unsigned bits = a == 0.f ? 0u : __float_as_uint(a);
  const unsigned mono = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  return order ? mono : ~mono;
}

// One workgroup per clip, as shap_ranks_kernel: the P keys go to LDS once, then every thread counts, for its cells, the
// keys before its own (a broadcast read).  A counting rank, not a sort.  With t_in == T != gt the cell value is the mean
// over the frames of the temporal cell: the fp32 sum in ascending u from 0.f, one division by the frame count.
__global__ __launch_bounds__(256) void curve_ranks_kernel(const float* __restrict__ a, int t_in, int T, int gt, int ghw,
                                                          int order, unsigned short* __restrict__ ranks) {
  __shared__ unsigned ks[CURVE_MAX_PLAYERS];
  const int P = gt * ghw;
  const float* ac = a + (size_t)blockIdx.x * t_in * ghw;
  for (int c = threadIdx.x; c < P; c += 256) {
    float v;
    if (t_in == gt) {
      v = ac[c];
    } else {
      const int kt = c / ghw, s = c - kt * ghw;
      float sum = 0.f;
      int cnt = 0;
      for (int u = 0; u < T; ++u)
        if ((u * gt) / T == kt) {
          sum += ac[(size_t)u * ghw + s];
          ++cnt;
        }
      v = sum / (float)cnt;      // gt <= T: every temporal cell has a frame
    }
    ks[c] = curve_key(v, order);
  }
  __syncthreads();
  unsigned short* out = ranks + (size_t)blockIdx.x * P;
  for (int c = threadIdx.x; c < P; c += 256) {
    const unsigned h = ks[c];
    int r = 0;
    for (int o = 0; o < P; ++o) {
      const unsigned v = ks[o];
      r += (v < h || (v == h && o < c)) ? 1 : 0;
    }
    out[c] = (unsigned short)r;
  }
}

// ---------------------------------------------------------------- staging
// row r of the flattened (clip, curve, j) list
struct CurveRow {
  int clip, ins, k;      // ins: the insertion test (rank >= k frozen); k the threshold
};
__device__ __forceinline__ CurveRow curve_row(long long r, const CurveGrid& g, int P) {
  const int per = g.ncurves * (g.J + 1);
  const int in_clip = (int)(r % per);
  const int ci = in_clip / (g.J + 1), j = in_clip - ci * (g.J + 1);
  const int ins = g.curves == 2 ? 1 : ci;            // curves 3: deletion first
  return {(int)(r / per), ins, (int)min((long long)j * g.step, (long long)P)};
}

// One workgroup per (row, 256 pixels): the row's gt * gh column words (bit jj = cell (kt, i, jj) frozen) are built once
// in LDS from the clip's rank table; every thread parks row x of A_W in its own LDS column.
struct CurveLds {
  unsigned* word;
  float* aw;
};

__device__ __forceinline__ CurveLds curve_fill_lds(unsigned* lds, const float* __restrict__ AW,
                                                   const unsigned short* __restrict__ rk, const CurveGrid& g,
                                                   const CurveRow& q, int x) {
  CurveLds l;
  l.word = lds;
  l.aw = reinterpret_cast<float*>(lds + g.gt * g.gh);
  const int tid = threadIdx.x;
  for (int w = tid; w < g.gt * g.gh; w += 256) {
    unsigned bits = 0;
    for (int j = 0; j < g.gw; ++j) {
      const bool below = (int)rk[w * g.gw + j] < q.k;
      bits |= ((below != (q.ins != 0)) ? 1u : 0u) << j;
    }
    l.word[w] = bits;
  }
  for (int j = 0; j < g.gw; ++j) l.aw[j * 256 + tid] = AW[(size_t)x * g.gw + j];
  __syncthreads();
  return l;
}

// tmp[i] = sum_{j set, ascending} A_W[x,j];  M = sum_{i ascending, all i} A_H[y,i] * tmp[i]: the expand's partial sums,
// which lose their zero terms exactly when S is binary.
__device__ __forceinline__ float curve_mask_at(const CurveLds& l, const float* __restrict__ AHy, int gh, int kt) {
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

// 16-byte channels-last pixels (C <= 4): with TT > 0 (T == TT) the 16 frames of a piece are requested before the scan
// goes over them.
template <int TT>   // 0, or a multiple of 16
__global__ __launch_bounds__(256) void curve_stage_cl4_kernel(const float* __restrict__ x, const float* __restrict__ AH,
                                                              const float* __restrict__ AW,
                                                              const unsigned short* __restrict__ ranks,
                                                              float* __restrict__ p, int C, int Trun, int W, int HW,
                                                              CurveGrid g, long long first) {
  extern __shared__ unsigned curve_lds[];
  const int row = blockIdx.y, T = TT > 0 ? TT : Trun, P = g.gt * g.gh * g.gw;
  const CurveRow q = curve_row(first + row, g, P);
  const int pxu = blockIdx.x * 256 + threadIdx.x;
  const int px = min(pxu, HW - 1);          // threads past the end stage LDS for a valid pixel, then leave
  const CurveLds l = curve_fill_lds(curve_lds, AW, ranks + (size_t)q.clip * P, g, q, px % W);
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
          m = curve_mask_at(l, AHy, g.gh, kt);
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
        m = curve_mask_at(l, AHy, g.gh, kt);
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
__global__ __launch_bounds__(256) void curve_stage_ncthw_kernel(const float* __restrict__ x, const float* __restrict__ AH,
                                                                const float* __restrict__ AW,
                                                                const unsigned short* __restrict__ ranks,
                                                                float* __restrict__ p, int C, int T, int W, int HW,
                                                                CurveGrid g, long long first) {
  extern __shared__ unsigned curve_lds[];
  const int row = blockIdx.y, P = g.gt * g.gh * g.gw;
  const CurveRow q = curve_row(first + row, g, P);
  const int pxu = blockIdx.x * 256 + threadIdx.x;
  const int px = min(pxu, HW - 1);
  const CurveLds l = curve_fill_lds(curve_lds, AW, ranks + (size_t)q.clip * P, g, q, px % W);
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
        m = curve_mask_at(l, AHy, g.gh, kt);
      }
      float xv = xp[(size_t)u * HW];
      float v = u ? (1.f - m) * xv + m * prev : xv;
      prev = v;
      pp[(size_t)u * HW] = v;
    }
  }
}

// ---------------------------------------------------------------- reduction
// One thread per (clip, curve) walks its J + 1 scores in ascending j: plain fp32, integer widths, one final division, no
// atomics, so a clip's numbers do not depend on the batch.  s_hi is the score of the clip, s_lo that of the fully
// frozen clip: the two ends of the curve, which end is which set by the curve's kind.
__global__ __launch_bounds__(256) void curve_reduce_kernel(const float* __restrict__ scores, int B, int ncurves,
                                                           int curves, int P, int step, int J, float* __restrict__ auc,
                                                           float* __restrict__ auc_norm) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * ncurves) return;
  const int ci = e % ncurves, ins = curves == 2 ? 1 : ci;
  const float* s = scores + (size_t)e * (J + 1);
  const float nan = __builtin_nanf("");
  float acc = 0.f;
  bool bad = s[0] != s[0];
  for (int j = 0; j < J; ++j) {
    const int k0 = j * step, k1 = min(k0 + step, P);
    const float z = s[j + 1];
    bad = bad || z != z;
    acc += (float)(k1 - k0) * (s[j] + z);
  }
  const float area = acc / (float)(2 * P);
  const float hi = ins ? s[J] : s[0], lo = ins ? s[0] : s[J];
  auc[e] = bad ? nan : area;
  auc_norm[e] = (bad || hi == lo) ? nan : (area - lo) / (hi - lo);
}

static bool curve_grid_ok(int T, int gt, int gh, int gw) {
  return T >= 1 && T <= MAX_T && gt >= 1 && gt <= T && gh >= 1 && gh <= CURVE_MAX_GRID && gw >= 1 && gw <= CURVE_MAX_GRID &&
         gt * gh * gw <= CURVE_MAX_PLAYERS;
}

#define CURVE_CHECK_GRID(what, T, gt, gh, gw)                                                                            \
  IVF_CHECK_ARG(curve_grid_ok(T, gt, gh, gw),                                                                            \
                what ": need 1 <= gt (%d) <= T (%d) <= %d, 1 <= gh (%d), gw (%d) <= %d and gt gh gw <= %d players", gt, T, \
                MAX_T, gh, gw, CURVE_MAX_GRID, CURVE_MAX_PLAYERS)

}  // namespace ivf

using namespace ivf;

extern "C" int ivf_curve_ranks(const float* a, int b, int t_in, int T, int gt, int gh, int gw, int order,
                               unsigned short* ranks, ivf_stream_t stream) {
  IVF_CHECK_ARG(a && ranks, "curve_ranks: null pointer");
  IVF_CHECK_ARG(b > 0, "curve_ranks: bad batch %d", b);
  CURVE_CHECK_GRID("curve_ranks", T, gt, gh, gw);
  IVF_CHECK_ARG(t_in == gt || t_in == T, "curve_ranks: t_in (%d) must be gt (%d) or T (%d)", t_in, gt, T);
  IVF_CHECK_ARG(order == 0 || order == 1, "curve_ranks: order must be 0 (most relevant first) or 1, got %d", order);
  hipLaunchKernelGGL(curve_ranks_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, a, t_in, T, gt, gh * gw, order, ranks);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_curve_stage(const float* x, int b, int C, int T, int H, int W, const float* A_H, const float* A_W,
                               int gt, int gh, int gw, const unsigned short* ranks, int curves, int step, long long first,
                               int count, float* p, int out_cpad, ivf_stream_t stream) {
  IVF_CHECK_ARG(x && A_H && A_W && ranks && p, "curve_stage: null pointer");
  IVF_CHECK_ARG(b > 0 && C > 0 && H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL, "curve_stage: bad dims");
  CURVE_CHECK_GRID("curve_stage", T, gt, gh, gw);
  const int P = gt * gh * gw;
  IVF_CHECK_ARG(curves >= 1 && curves <= 3, "curve_stage: curves must be 1 (deletion), 2 (insertion) or 3 (both), got %d",
                curves);
  IVF_CHECK_ARG(step >= 1 && step <= P, "curve_stage: step %d outside 1 .. %d cells", step, P);
  const int J = (P + step - 1) / step, nc = curves == 3 ? 2 : 1;
  const long long rows = (long long)b * nc * (J + 1);
  IVF_CHECK_ARG(first >= 0 && count > 0 && count <= 65535 && first + count <= rows,
                "curve_stage: rows [%lld, %lld) outside the %lld rows of %d clips (at most 65535 rows a call)", first,
                first + count, rows, b);
  IVF_CHECK_ARG(out_cpad == 0 || (out_cpad == 4 && C <= 4),
                "curve_stage: out_cpad must be 0 (NCTHW) or 4 (16-byte channels-last, C <= 4)");
  IVF_CHECK_ARG(out_cpad == 0 || ((uintptr_t)p & 15) == 0, "curve_stage: the channels-last buffer is not 16-byte aligned");
  const CurveGrid g{gt, gh, gw, curves, nc, step, J};
  const int HW = H * W;
  const size_t lds = ((size_t)gt * gh + (size_t)gw * 256) * 4;      // at most 8 + 32 KiB
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(cdiv(HW, 256), count), block(256);
  if (out_cpad == 0)
    hipLaunchKernelGGL(curve_stage_ncthw_kernel, grid, block, lds, s, x, A_H, A_W, ranks, p, C, T, W, HW, g, first);
  else
    with_frames_exact(T, [&](auto TT) {
      hipLaunchKernelGGL(curve_stage_cl4_kernel<TT>, grid, block, lds, s, x, A_H, A_W, ranks, p, C, T, W, HW, g, first);
    });
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_curve_reduce(const float* scores, int b, int ncurves, int curves, int P, int step, float* auc,
                                float* auc_norm, ivf_stream_t stream) {
  IVF_CHECK_ARG(scores && auc && auc_norm, "curve_reduce: null pointer");
  IVF_CHECK_ARG(curves >= 1 && curves <= 3, "curve_reduce: curves must be 1 (deletion), 2 (insertion) or 3 (both), got %d",
                curves);
  IVF_CHECK_ARG(ncurves == (curves == 3 ? 2 : 1), "curve_reduce: curves %d names %d curves, not %d", curves,
                curves == 3 ? 2 : 1, ncurves);
  IVF_CHECK_ARG(b > 0 && (long long)b * ncurves <= 0x7fffffffLL - 255, "curve_reduce: bad batch %d", b);
  IVF_CHECK_ARG(P >= 1 && P <= CURVE_MAX_PLAYERS, "curve_reduce: %d players outside 1 .. %d", P, CURVE_MAX_PLAYERS);
  IVF_CHECK_ARG(step >= 1 && step <= P, "curve_reduce: step %d outside 1 .. %d cells", step, P);
  const int J = (P + step - 1) / step;
  hipLaunchKernelGGL(curve_reduce_kernel, dim3(cdiv(b * ncurves, 256)), dim3(256), 0, (hipStream_t)stream, scores, b,
                     ncurves, curves, P, step, J, auc, auc_norm);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}
