// Shapley value sampling for video (Castro et al. 2009; Strumbelj & Kononenko 2014), an EXTENSION with no counterpart
// in the reference.  The players are the cells of a grid (gt, gh, gw), a coalition is the set of frozen
// cells, its value the class score of the clip frozen per pixel by that binary mask.  Permutation sampling: along
// permutation k the cells are frozen one after another, prefix j = the j cells of lowest rank frozen, and the marginal
// of cell c is the score drop on its entry,
//   d_k[c] = s[k][rank_k[c]] - s[k][rank_k[c] + 1],         phi[c] = mean_k d_k[c]     (phi > 0: freezing c lowers the score)
// so that sum_c d_k[c] = s[k][0] - s[k][P] telescopes for every k: the clip's score minus the fully frozen clip's.
//
// The permutation family is integer-exact and the same for every clip.  With the hash of the RISE masks (grid_stage.h),
//   h(seed, k, c) = grid_hash(grid_key(seed, k), c)                                                   (uint32, wrapping)
//   rank_k[c] = #{c' : (h(seed,k,c'), c') < (h(seed,k,c), c)}                        (lexicographic: a tie falls to the lower index)
// and, antithetic, an odd k is permutation k - 1 (hashed as itself) reversed: rank_k[c] = P - 1 - rank_{k-1}[c].
//
// Row (clip, k, j) freezes the cells with rank_k[c] < j.  The staging kernels and their scan are the shared ones of
// grid_stage.h; this file gives them the rows (a rank table, not a threshold).
#include "grid_stage.h"

namespace ivf {

// ---------------------------------------------------------------- rank table
// One workgroup per permutation: the P hashes go to LDS once, then every thread counts, for its cells, the hashes below
// its own (grid_count_rank).  At P = 4096 that is 2^24 compares per permutation, 65,536 per thread: 1.6 ms for 64
// permutations (measured), once per call, beside n (P + 1) forward passes.
__global__ __launch_bounds__(256) void shap_ranks_kernel(unsigned seed, int antithetic, int first_k, int P,
                                                         unsigned short* __restrict__ ranks) {
  __shared__ unsigned hs[GRID_MAX_PLAYERS];
  const int k = first_k + blockIdx.x;
  const bool rev = antithetic && (k & 1);
  const unsigned key = grid_key(seed, rev ? k - 1 : k);
  for (int c = threadIdx.x; c < P; c += 256) hs[c] = grid_hash(key, c);
  __syncthreads();
  unsigned short* out = ranks + (size_t)blockIdx.x * P;
  for (int c = threadIdx.x; c < P; c += 256) {
    const int r = grid_count_rank(hs, P, c);
    out[c] = (unsigned short)(rev ? P - 1 - r : r);
  }
}

// ---------------------------------------------------------------- staging
// row r of the flattened (clip, permutation, prefix) list: cell c frozen iff its rank is below the prefix length
struct ShapRows {
  int n;                                       // permutations per clip; a clip has n (P + 1) rows
  const unsigned short* __restrict__ ranks;    // [n,P]
  struct Cells {
    int clip, prefix;
    const unsigned short* __restrict__ rk;
    __device__ __forceinline__ bool frozen(int c) const { return (int)rk[c] < prefix; }
  };
  __device__ __forceinline__ Cells cells(long long r, int P) const {
    const long long per = (long long)n * (P + 1);
    const int in_clip = (int)(r % per), k = in_clip / (P + 1);
    return {(int)(r / per), in_clip % (P + 1), ranks + (size_t)k * P};
  }
};

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

}  // namespace ivf

using namespace ivf;

extern "C" int ivf_shap_ranks(unsigned seed, int antithetic, int first_k, int count, int gt, int gh, int gw,
                              unsigned short* ranks, ivf_stream_t stream) {
  IVF_CHECK_ARG(ranks, "shap_ranks: null pointer");
  // the clip length is not this entry's: gt <= MAX_T
  IVF_PROPAGATE(grid_check("shap_ranks", MAX_T, gt, gh, gw, GRID_MAX_PLAYERS));
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
  const GridStageArgs a{"shap_stage", x, b, C, T, H, W, A_H, A_W, {gt, gh, gw}, first, count, p, out_cpad, stream};
  IVF_PROPAGATE(grid_stage_check(a, ranks != nullptr, GRID_MAX_PLAYERS));
  IVF_CHECK_ARG(n > 0 && (long long)n * (gt * gh * gw + 1) <= 0x7fffffffLL, "shap_stage: bad permutation count %d", n);
  return grid_stage_launch(a, ShapRows{n, ranks}, (long long)b * n * (gt * gh * gw + 1), "rows");
}

extern "C" int ivf_shap_reduce(const float* scores, const unsigned short* ranks, int b, int n, int gt, int gh, int gw,
                               float* cells, float* stderr_out, int* count, float* total, ivf_stream_t stream) {
  IVF_CHECK_ARG(scores && ranks && cells && stderr_out && count && total, "shap_reduce: null pointer");
  IVF_CHECK_ARG(b > 0 && n > 0, "shap_reduce: bad batch %d or permutation count %d", b, n);
  IVF_PROPAGATE(grid_check("shap_reduce", MAX_T, gt, gh, gw, GRID_MAX_PLAYERS));
  const int P = gt * gh * gw;
  const long long all = (long long)b * P;
  IVF_CHECK_ARG((all + 255) / 256 <= 0x7fffffffLL, "shap_reduce: too many cells");
  hipLaunchKernelGGL(shap_reduce_kernel, dim3(cdiv(all, 256)), dim3(256), 0, (hipStream_t)stream, scores, ranks, b, n, P,
                     cells, stderr_out, count, total);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}
