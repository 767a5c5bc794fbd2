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
// The staging kernels and their scan are the shared ones of grid_stage.h; this file gives them the rows: a per-clip rank
// table, a threshold of several cells, and the insertion test.  Rows are flattened as [clip][curve][j], so a chunk of the
// plan's batch crosses clip and curve boundaries.
//
// Reduction.  auc = (1 / (2P)) sum_{j<J} (k_{j+1} - k_j) (s_j + s_{j+1}): the trapezoid over the fraction of cells.
#include "grid_stage.h"

namespace ivf {

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
// keys before its own (grid_count_rank).  With t_in == T != gt the cell value is the mean over the frames of the
// temporal cell: the fp32 sum in ascending u from 0.f, one division by the frame count.
__global__ __launch_bounds__(256) void curve_ranks_kernel(const float* __restrict__ a, int t_in, int T, int gt, int ghw,
                                                          int order, unsigned short* __restrict__ ranks) {
  __shared__ unsigned ks[GRID_MAX_PLAYERS];
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
  for (int c = threadIdx.x; c < P; c += 256) out[c] = (unsigned short)grid_count_rank(ks, P, c);
}

// ---------------------------------------------------------------- staging
// row r of the flattened (clip, curve, j) list: cell c frozen iff (rank[c] < k_j) != insertion
struct CurveRows {
  int curves, ncurves;   // bit 0 deletion, bit 1 insertion; ncurves = their number
  int step, J;           // a clip has ncurves (J + 1) rows
  const unsigned short* __restrict__ ranks;    // [b,P]
  struct Cells {
    int clip, ins, k;      // ins: the insertion test (rank >= k frozen); k the threshold
    const unsigned short* __restrict__ rk;
    __device__ __forceinline__ bool frozen(int c) const {
      const bool below = (int)rk[c] < k;
      return below != (ins != 0);
    }
  };
  __device__ __forceinline__ Cells cells(long long r, int P) const {
    const int per = ncurves * (J + 1);
    const int in_clip = (int)(r % per), clip = (int)(r / per);
    const int ci = in_clip / (J + 1), j = in_clip - ci * (J + 1);
    const int ins = curves == 2 ? 1 : ci;            // curves 3: deletion first
    return {clip, ins, (int)min((long long)j * step, (long long)P), ranks + (size_t)clip * P};
  }
};

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

}  // namespace ivf

using namespace ivf;

extern "C" int ivf_curve_ranks(const float* a, int b, int t_in, int T, int gt, int gh, int gw, int order,
                               unsigned short* ranks, ivf_stream_t stream) {
  IVF_CHECK_ARG(a && ranks, "curve_ranks: null pointer");
  IVF_CHECK_ARG(b > 0, "curve_ranks: bad batch %d", b);
  IVF_PROPAGATE(grid_check("curve_ranks", T, gt, gh, gw, GRID_MAX_PLAYERS));
  IVF_CHECK_ARG(t_in == gt || t_in == T, "curve_ranks: t_in (%d) must be gt (%d) or T (%d)", t_in, gt, T);
  IVF_CHECK_ARG(order == 0 || order == 1, "curve_ranks: order must be 0 (most relevant first) or 1, got %d", order);
  hipLaunchKernelGGL(curve_ranks_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, a, t_in, T, gt, gh * gw, order, ranks);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_curve_stage(const float* x, int b, int C, int T, int H, int W, const float* A_H, const float* A_W,
                               int gt, int gh, int gw, const unsigned short* ranks, int curves, int step, long long first,
                               int count, float* p, int out_cpad, ivf_stream_t stream) {
  const GridStageArgs a{"curve_stage", x, b, C, T, H, W, A_H, A_W, {gt, gh, gw}, first, count, p, out_cpad, stream};
  IVF_PROPAGATE(grid_stage_check(a, ranks != nullptr, GRID_MAX_PLAYERS));
  const int P = gt * gh * gw;
  IVF_CHECK_ARG(curves >= 1 && curves <= 3, "curve_stage: curves must be 1 (deletion), 2 (insertion) or 3 (both), got %d",
                curves);
  IVF_CHECK_ARG(step >= 1 && step <= P, "curve_stage: step %d outside 1 .. %d cells", step, P);
  const int J = (P + step - 1) / step, nc = curves == 3 ? 2 : 1;
  return grid_stage_launch(a, CurveRows{curves, nc, step, J, ranks}, (long long)b * nc * (J + 1), "rows");
}

extern "C" int ivf_curve_reduce(const float* scores, int b, int ncurves, int curves, int P, int step, float* auc,
                                float* auc_norm, ivf_stream_t stream) {
  IVF_CHECK_ARG(scores && auc && auc_norm, "curve_reduce: null pointer");
  IVF_CHECK_ARG(curves >= 1 && curves <= 3, "curve_reduce: curves must be 1 (deletion), 2 (insertion) or 3 (both), got %d",
                curves);
  IVF_CHECK_ARG(ncurves == (curves == 3 ? 2 : 1), "curve_reduce: curves %d names %d curves, not %d", curves,
                curves == 3 ? 2 : 1, ncurves);
  IVF_CHECK_ARG(b > 0 && (long long)b * ncurves <= 0x7fffffffLL - 255, "curve_reduce: bad batch %d", b);
  IVF_CHECK_ARG(P >= 1 && P <= GRID_MAX_PLAYERS, "curve_reduce: %d players outside 1 .. %d", P, GRID_MAX_PLAYERS);
  IVF_CHECK_ARG(step >= 1 && step <= P, "curve_reduce: step %d outside 1 .. %d cells", step, P);
  const int J = (P + step - 1) / step;
  hipLaunchKernelGGL(curve_reduce_kernel, dim3(cdiv(b * ncurves, 256)), dim3(256), 0, (hipStream_t)stream, scores, b,
                     ncurves, curves, P, step, J, auc, auc_norm);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}
