// Linear surrogates for video: KernelSHAP (Lundberg & Lee 2017) and LIME (Ribeiro et al. 2016), an EXTENSION with no
// counterpart in the reference.  The players are the cells of a grid (gt, gh, gw), a sample row freezes a
// set of cells, its value is the class score of the clip frozen per pixel by that binary mask, and a linear model of
// the score drop y = score_x - score in the frozen cells is fitted by least squares:
//   KernelSHAP  the coalition sizes are drawn from the Shapley kernel (so the rows weigh 1), the efficiency constraint
//               sum phi = score_x - score(all frozen) is eliminated exactly through the last cell;
//   LIME        Bernoulli rows (RISE's masks), weighted by an exponential kernel of the distance to the clip, a ridge
//               penalty and a free intercept.
// The rows are integer-exact and the same for every clip (the hash and the counting rank of grid_stage.h); they are
// kept as packed bits [n, ceil(P/32)].  The staging kernels and their scan are the shared ones of grid_stage.h; this
// file gives them the rows (a bit table).  The fit is fp64 on the device: moments with one ascending-k chain per
// element, a blocked right-looking Cholesky factorisation, forward and back substitution -- every sum in a fixed order,
// no atomics, so a clip's numbers depend neither on the batch nor on the run.
#include <algorithm>

#include "grid_stage.h"

namespace ivf {

constexpr int LIN_NB = 32;                 // Cholesky block: a diagonal block is 8 KiB of LDS
constexpr int LIN_MAX_ROWS = 1 << 20;      // sample rows of a call

static inline int lin_words(int P) { return (P + 31) >> 5; }

// ---------------------------------------------------------------- rows
// One workgroup per row.  A wave's ballot is the 64 consecutive cells of two words: no atomics, and a lane beyond P
// votes 0, so the unused high bits are zero.
__device__ __forceinline__ void lin_put_bits(unsigned* __restrict__ out, int nw, int c, bool f) {
  const unsigned long long m = __ballot(f);
  if ((threadIdx.x & 63) == 0) {
    const int w = c >> 5;
    if (w < nw) out[w] = (unsigned)m;
    if (w + 1 < nw) out[w + 1] = (unsigned)(m >> 32);
  }
}

// KernelSHAP: the P rank hashes go to LDS (shap_ranks_kernel's table), the size comes from the hash of the cell index
// P, which the ranks never use, by integer compares against the caller's table.
__global__ __launch_bounds__(256) void kshap_rows_kernel(unsigned seed, int paired, int first_k, int P,
                                                         const unsigned* __restrict__ size_table,
                                                         unsigned* __restrict__ bits, unsigned short* __restrict__ sizes) {
  __shared__ unsigned hs[LIN_MAX_PLAYERS];
  const int k = first_k + blockIdx.x, tid = threadIdx.x;
  const bool odd = paired && (k & 1);
  const unsigned key = grid_key(seed, odd ? k - 1 : k);
  for (int c = tid; c < P; c += 256) hs[c] = grid_hash(key, c);
  const unsigned h = grid_hash(key, P);
  int s = 1;
  for (int i = 0; i < P - 2; ++i) s += h >= size_table[i] ? 1 : 0;
  if (odd) s = P - s;
  __syncthreads();
  const int nw = (P + 31) >> 5;
  unsigned* out = bits + (size_t)blockIdx.x * nw;
  for (int c0 = 0; c0 < P; c0 += 256) {
    const int c = c0 + tid;
    bool f = false;
    if (c < P) {
      const int r = grid_count_rank(hs, P, c);
      f = (odd ? P - 1 - r : r) < s;
    }
    lin_put_bits(out, nw, c, f);
  }
  if (tid == 0) sizes[blockIdx.x] = (unsigned short)s;
}

__global__ __launch_bounds__(256) void lime_rows_kernel(unsigned seed, unsigned thresh, int first_k, int P,
                                                        unsigned* __restrict__ bits) {
  const int tid = threadIdx.x;
  const unsigned key = grid_key(seed, first_k + blockIdx.x);
  const int nw = (P + 31) >> 5;
  unsigned* out = bits + (size_t)blockIdx.x * nw;
  for (int c0 = 0; c0 < P; c0 += 256) {
    const int c = c0 + tid;
    lin_put_bits(out, nw, c, c < P && grid_hash(key, c) < thresh);
  }
}

// ---------------------------------------------------------------- staging
// row r of the flattened (clip, row) list: a clip has its n sample rows and row n, every cell frozen
struct BitRows {
  int n, nw;
  const unsigned* __restrict__ bits;    // [n,nw]
  struct Cells {
    int clip;
    const unsigned* __restrict__ w;     // null: row n
    __device__ __forceinline__ bool frozen(int c) const { return !w || ((w[c >> 5] >> (c & 31)) & 1u); }
  };
  __device__ __forceinline__ Cells cells(long long r, int) const {
    const int in_clip = (int)(r % (n + 1));
    return {(int)(r / (n + 1)), in_clip == n ? nullptr : bits + (size_t)in_clip * nw};
  }
};

// ---------------------------------------------------------------- moments
__device__ __forceinline__ bool lin_bit(const unsigned* __restrict__ bits, int nw, int k, int c) {
  return (bits[(size_t)k * nw + (c >> 5)] >> (c & 31)) & 1u;
}

// w_k of every row, one thread a row
__global__ __launch_bounds__(256) void lin_wrow_kernel(const unsigned* __restrict__ bits, const double* __restrict__ wtab,
                                                       int n, int nw, double* __restrict__ wrow) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  int m = 0;
  for (int w = 0; w < nw; ++w) m += __popc(bits[(size_t)k * nw + w]);
  wrow[k] = wtab ? wtab[m] : 1.0;
}

// one workgroup per clip
__global__ __launch_bounds__(256) void lin_ok_kernel(const float* __restrict__ scores, const float* __restrict__ score_x,
                                                     int n, int* __restrict__ ok) {
  const int b = blockIdx.x;
  int good = __builtin_isfinite(score_x[b]) ? 1 : 0;
  for (int k = threadIdx.x; k <= n; k += 256) good &= __builtin_isfinite(scores[(size_t)b * (n + 1) + k]) ? 1 : 0;
  good = __syncthreads_and(good);
  if (threadIdx.x == 0) ok[b] = good ? 1 : 0;
}

// N: one thread per (c, c'), a workgroup a 16 x 16 tile -- its 16 + 16 cells lie in one word each, so a row's two
// words are the same for the whole workgroup
__global__ __launch_bounds__(256) void lin_N_kernel(const unsigned* __restrict__ bits, const double* __restrict__ wrow,
                                                    int n, int nw, int P, double* __restrict__ N) {
  const int c = blockIdx.y * 16 + (threadIdx.x >> 4), d = blockIdx.x * 16 + (threadIdx.x & 15);
  const int wc = (blockIdx.y * 16) >> 5, wd = (blockIdx.x * 16) >> 5;      // below nw: the tile starts below P
  const int sc = c & 31, sd = d & 31;
  double acc = 0.0;
  for (int k = 0; k < n; ++k) {
    const unsigned a = bits[(size_t)k * nw + wc], e = bits[(size_t)k * nw + wd];
    if ((a >> sc) & (e >> sd) & 1u) acc += wrow[k];
  }
  if (c < P && d < P) N[(size_t)c * P + d] = acc;
}

// v, Wsum, r, t: one thread per (j, c), j = 0 the weights themselves (v; c == P: Wsum), j >= 1 clip j - 1 (r; c == P: t)
__global__ __launch_bounds__(256) void lin_vr_kernel(const float* __restrict__ scores, const float* __restrict__ score_x,
                                                     const unsigned* __restrict__ bits, const double* __restrict__ wrow,
                                                     int B, int n, int nw, int P, double* __restrict__ v,
                                                     double* __restrict__ Wsum, double* __restrict__ r,
                                                     double* __restrict__ t) {
  const size_t e = blockIdx.x * (size_t)256 + threadIdx.x;
  if (e >= (size_t)(B + 1) * (P + 1)) return;
  const int j = (int)(e / (P + 1)), c = (int)(e - (size_t)j * (P + 1));
  double acc = 0.0;
  if (j == 0) {
    for (int k = 0; k < n; ++k)
      if (c == P || lin_bit(bits, nw, k, c)) acc += wrow[k];
    if (c == P) Wsum[0] = acc;
    else v[c] = acc;
  } else {
    const float* s = scores + (size_t)(j - 1) * (n + 1);
    const double sx = (double)score_x[j - 1];
    for (int k = 0; k < n; ++k)
      if (c == P || lin_bit(bits, nw, k, c)) {
        const double wy = wrow[k] * (sx - (double)s[k]);
        acc += wy;
      }
    if (c == P) t[j - 1] = acc;
    else r[(size_t)(j - 1) * P + c] = acc;
  }
}

// ---------------------------------------------------------------- system
// The caller's workspace: A [m,m] (row-major, the lower triangle is the factor's), diag0 [P] (the diagonal before the
// factorisation), mu [P], and the singular flag.
struct LinWork {
  double *A, *diag0, *mu;
  int* flag;
  LinWork(void* w, int P) {
    A = (double*)w;
    diag0 = A + (size_t)P * P;
    mu = diag0 + P;
    flag = (int*)(mu + P);
  }
  static size_t bytes(int P) { return ((size_t)P * P + 2 * (size_t)P + 1) * 8; }
};

__global__ __launch_bounds__(256) void lin_assemble_kernel(int kind, const double* __restrict__ N,
                                                           const double* __restrict__ v, const double* __restrict__ Wsum,
                                                           int P, int m, double ridge, double* __restrict__ A,
                                                           double* __restrict__ diag0, double* __restrict__ mu,
                                                           int* __restrict__ flag) {
  const size_t e = blockIdx.x * (size_t)256 + threadIdx.x;
  if (e == 0) *flag = 0;
  if (e >= (size_t)m * m) return;
  const int c = (int)(e / m), d = (int)(e - (size_t)c * m);
  double a;
  if (kind == 0) {
    const int l = P - 1;
    a = ((N[(size_t)c * P + d] - N[(size_t)c * P + l]) - N[(size_t)l * P + d]) + N[(size_t)l * P + l];
  } else {
    const double W = Wsum[0], mc = v[c] / W, md = v[d] / W;
    const double mm = mc * md;
    a = N[(size_t)c * P + d] - W * mm;
    if (c == d) a += ridge;
    if (d == 0) mu[c] = mc;
  }
  A[e] = a;
  if (c == d) diag0[c] = a;
}

// ---------------------------------------------------------------- Cholesky, blocked and right-looking
// Block column [j0, j0 + nb): the diagonal block is factored by one workgroup in LDS (lin_potrf_kernel), the panel
// below it is solved against the block's factor one row a thread (lin_trsm_kernel), and every 32 x 32 tile of the
// trailing lower triangle loses the panel's product (lin_syrk_kernel).  An element's subtractions run in ascending
// column order, each product rounded before it is subtracted.
__global__ __launch_bounds__(256) void lin_potrf_kernel(double* __restrict__ A, int m, int j0, int nb,
                                                        const double* __restrict__ diag0, int* __restrict__ flag) {
  __shared__ double a[LIN_NB][LIN_NB + 1];
  const int tid = threadIdx.x;
  for (int e = tid; e < LIN_NB * LIN_NB; e += 256) {
    const int i = e >> 5, k = e & 31;
    a[i][k] = (i < nb && k <= i) ? A[(size_t)(j0 + i) * m + j0 + k] : 0.0;
  }
  __syncthreads();
  for (int p = 0; p < nb; ++p) {
    if (tid == 0) {
      const double d = a[p][p];
      if (!(d > 0x1p-20 * diag0[j0 + p]) || !__builtin_isfinite(d)) *flag = 1;
      a[p][p] = sqrt(d);
    }
    __syncthreads();
    if (tid > p && tid < nb) a[tid][p] = a[tid][p] / a[p][p];
    __syncthreads();
    for (int e = tid; e < LIN_NB * LIN_NB; e += 256) {
      const int i = e >> 5, k = e & 31;
      if (k > p && k <= i && i < nb) a[i][k] -= a[i][p] * a[k][p];
    }
    __syncthreads();
  }
  for (int e = tid; e < LIN_NB * LIN_NB; e += 256) {
    const int i = e >> 5, k = e & 31;
    if (i < nb && k <= i) A[(size_t)(j0 + i) * m + j0 + k] = a[i][k];
  }
}

__global__ __launch_bounds__(64) void lin_trsm_kernel(double* __restrict__ A, int m, int j0, int nb) {
  __shared__ double l[LIN_NB][LIN_NB + 1];
  __shared__ double xs[64][LIN_NB + 1];
  const int tid = threadIdx.x;
  for (int e = tid; e < LIN_NB * LIN_NB; e += 64) {
    const int i = e >> 5, k = e & 31;
    l[i][k] = (i < nb && k <= i) ? A[(size_t)(j0 + i) * m + j0 + k] : 0.0;
  }
  __syncthreads();
  const int i = j0 + nb + blockIdx.x * 64 + tid;
  if (i >= m) return;
  double* row = A + (size_t)i * m + j0;
  for (int p = 0; p < nb; ++p) {
    double acc = row[p];
    for (int q = 0; q < p; ++q) acc -= xs[tid][q] * l[p][q];
    xs[tid][p] = acc / l[p][p];
  }
  for (int p = 0; p < nb; ++p) row[p] = xs[tid][p];
}

// tile (blockIdx.y, blockIdx.x) of the trailing matrix that starts at j1 = j0 + nb; tiles above the diagonal leave
__global__ __launch_bounds__(256) void lin_syrk_kernel(double* __restrict__ A, int m, int j0, int nb) {
  if (blockIdx.x > blockIdx.y) return;
  __shared__ double li[LIN_NB][LIN_NB + 1];
  __shared__ double lk[LIN_NB][LIN_NB + 1];
  const int tid = threadIdx.x, j1 = j0 + nb;
  const int i0 = j1 + blockIdx.y * LIN_NB, k0 = j1 + blockIdx.x * LIN_NB;
  for (int e = tid; e < LIN_NB * LIN_NB; e += 256) {
    const int i = e >> 5, p = e & 31;
    li[i][p] = (i0 + i < m && p < nb) ? A[(size_t)(i0 + i) * m + j0 + p] : 0.0;
    lk[i][p] = (k0 + i < m && p < nb) ? A[(size_t)(k0 + i) * m + j0 + p] : 0.0;
  }
  __syncthreads();
  for (int e = tid; e < LIN_NB * LIN_NB; e += 256) {
    const int i = e >> 5, k = e & 31;
    const int gi = i0 + i, gk = k0 + k;
    if (gi >= m || gk > gi) continue;
    double acc = A[(size_t)gi * m + gk];
    for (int p = 0; p < nb; ++p) acc -= li[i][p] * lk[k][p];
    A[(size_t)gi * m + gk] = acc;
  }
}

// ---------------------------------------------------------------- substitution and outputs
// One workgroup per clip: the right-hand side is built in LDS, L y = rhs forward and L^T phi = y backward in blocks of
// LIN_NB columns (the block's triangle one column a step, then every row beyond it takes the block's products in
// order), then the outputs, each the fp64 value rounded once.
__global__ __launch_bounds__(256) void lin_subst_kernel(int kind, const double* __restrict__ A, int m,
                                                        const double* __restrict__ N, const double* __restrict__ r,
                                                        const double* __restrict__ t, const double* __restrict__ Wsum,
                                                        const double* __restrict__ mu, const float* __restrict__ scores,
                                                        const float* __restrict__ score_x, int n, int P,
                                                        const int* __restrict__ flag, int* __restrict__ ok,
                                                        float* __restrict__ cells, float* __restrict__ intercept,
                                                        float* __restrict__ total) {
  __shared__ double y[LIN_MAX_PLAYERS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const double total_b = (double)score_x[b] - (double)scores[(size_t)b * (n + 1) + n];
  const bool good = ok[b] != 0 && *flag == 0;
  float* out = cells + (size_t)b * P;
  if (!good) {
    const float nan = __builtin_nanf("");
    for (int c = tid; c < P; c += 256) out[c] = nan;
    if (tid == 0) {
      intercept[b] = nan;
      total[b] = (float)total_b;
      ok[b] = 0;
    }
    return;
  }
  const int l = P - 1;
  for (int c = tid; c < m; c += 256) {
    if (kind == 0) {
      const double dn = N[(size_t)c * P + l] - N[(size_t)l * P + l];
      y[c] = (r[(size_t)b * P + c] - r[(size_t)b * P + l]) - total_b * dn;
    } else {
      y[c] = r[(size_t)b * P + c] - mu[c] * t[b];
    }
  }
  __syncthreads();
  for (int j0 = 0; j0 < m; j0 += LIN_NB) {
    const int nb = min(LIN_NB, m - j0);
    for (int p = 0; p < nb; ++p) {
      const int j = j0 + p;
      if (tid == 0) y[j] = y[j] / A[(size_t)j * m + j];
      __syncthreads();
      if (tid > p && tid < nb) y[j0 + tid] -= A[(size_t)(j0 + tid) * m + j] * y[j];
      __syncthreads();
    }
    for (int i = j0 + nb + tid; i < m; i += 256) {
      double acc = y[i];
      for (int p = 0; p < nb; ++p) acc -= A[(size_t)i * m + j0 + p] * y[j0 + p];
      y[i] = acc;
    }
    __syncthreads();
  }
  for (int j0 = ((m - 1) / LIN_NB) * LIN_NB; j0 >= 0; j0 -= LIN_NB) {
    const int nb = min(LIN_NB, m - j0);
    for (int p = nb - 1; p >= 0; --p) {
      const int j = j0 + p;
      if (tid == 0) y[j] = y[j] / A[(size_t)j * m + j];
      __syncthreads();
      if (tid < p) y[j0 + tid] -= A[(size_t)j * m + j0 + tid] * y[j];
      __syncthreads();
    }
    for (int i = tid; i < j0; i += 256) {
      double acc = y[i];
      for (int p = nb - 1; p >= 0; --p) acc -= A[(size_t)(j0 + p) * m + i] * y[j0 + p];
      y[i] = acc;
    }
    __syncthreads();
  }
  for (int c = tid; c < m; c += 256) out[c] = (float)y[c];
  if (tid == 0) {
    double acc = 0.0;
    if (kind == 0) {
      for (int c = 0; c < m; ++c) acc += y[c];
      out[l] = (float)(total_b - acc);
      intercept[b] = 0.f;
    } else {
      for (int c = 0; c < m; ++c) acc += mu[c] * y[c];
      intercept[b] = (float)(t[b] / Wsum[0] - acc);
    }
    total[b] = (float)total_b;
  }
}

// ---------------------------------------------------------------- fit quality
// One workgroup per clip: 256 rows at a time every thread forms its row's two terms, then thread 0 adds them to the
// two chains in ascending k.
__global__ __launch_bounds__(256) void lin_fit_kernel(const float* __restrict__ scores, const float* __restrict__ score_x,
                                                      const unsigned* __restrict__ bits, const double* __restrict__ wrow,
                                                      const float* __restrict__ cells, const float* __restrict__ intercept,
                                                      const double* __restrict__ t, const double* __restrict__ Wsum,
                                                      const int* __restrict__ ok, int n, int nw, int P,
                                                      float* __restrict__ r2) {
  __shared__ double num[256], den[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (!ok[b]) {
    if (tid == 0) r2[b] = __builtin_nanf("");
    return;
  }
  const float* s = scores + (size_t)b * (n + 1);
  const float* phi = cells + (size_t)b * P;
  const double sx = (double)score_x[b], ybar = t[b] / Wsum[0], a0 = intercept ? (double)intercept[b] : 0.0;
  double snum = 0.0, sden = 0.0;
  for (int k0 = 0; k0 < n; k0 += 256) {
    const int k = k0 + tid;
    if (k < n) {
      double yh = a0;
      for (int c = 0; c < P; ++c)
        if (lin_bit(bits, nw, k, c)) yh += (double)phi[c];
      const double w = wrow ? wrow[k] : 1.0, yk = sx - (double)s[k];
      const double e1 = yk - yh, e2 = yk - ybar;
      num[tid] = w * (e1 * e1);
      den[tid] = w * (e2 * e2);
    }
    __syncthreads();
    if (tid == 0) {
      const int cnt = min(256, n - k0);
      for (int q = 0; q < cnt; ++q) {
        snum += num[q];
        sden += den[q];
      }
    }
    __syncthreads();
  }
  if (tid == 0) r2[b] = sden == 0.0 ? __builtin_nanf("") : (float)(1.0 - snum / sden);
}

// the grid of a rows entry: its clip length is not the entry's (gt <= MAX_T), 2 <= P <= LIN_MAX_PLAYERS
static inline int lin_rows_check(const char* name, int gt, int gh, int gw, int first_k, int count) {
  IVF_PROPAGATE(grid_check(name, MAX_T, gt, gh, gw, LIN_MAX_PLAYERS));
  IVF_CHECK_ARG(gt * gh * gw >= 2, "%s: need at least 2 players, got grid (%d, %d, %d)", name, gt, gh, gw);
  IVF_CHECK_ARG(first_k >= 0 && count > 0 && (long long)first_k + count <= 0x7fffffffLL,
                "%s: rows [%d, %lld) outside 0 .. 2^31 - 1", name, first_k, (long long)first_k + count);
  return IVF_OK;
}

}  // namespace ivf

using namespace ivf;

extern "C" int ivf_kshap_rows(unsigned seed, int paired, int first_k, int count, int gt, int gh, int gw,
                              const unsigned* size_table, unsigned* bits, unsigned short* sizes, ivf_stream_t stream) {
  IVF_CHECK_ARG(bits && sizes, "kshap_rows: null pointer");
  IVF_PROPAGATE(lin_rows_check("kshap_rows", gt, gh, gw, first_k, count));
  const int P = gt * gh * gw;
  IVF_CHECK_ARG(size_table || P == 2, "kshap_rows: null pointer (size_table, %d players)", P);
  IVF_CHECK_ARG(paired == 0 || paired == 1, "kshap_rows: paired must be 0 or 1, got %d", paired);
  hipLaunchKernelGGL(kshap_rows_kernel, dim3(count), dim3(256), 0, (hipStream_t)stream, seed, paired, first_k, P,
                     size_table, bits, sizes);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_lime_rows(unsigned seed, unsigned thresh, int first_k, int count, int gt, int gh, int gw, unsigned* bits,
                             ivf_stream_t stream) {
  IVF_CHECK_ARG(bits, "lime_rows: null pointer");
  IVF_PROPAGATE(lin_rows_check("lime_rows", gt, gh, gw, first_k, count));
  IVF_CHECK_ARG(thresh != 0, "lime_rows: thresh must be > 0 (thresh = floor(p 2^32), 0 < p < 1)");
  hipLaunchKernelGGL(lime_rows_kernel, dim3(count), dim3(256), 0, (hipStream_t)stream, seed, thresh, first_k,
                     gt * gh * gw, bits);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_lin_stage(const float* x, int b, int C, int T, int H, int W, const float* A_H, const float* A_W, int gt,
                             int gh, int gw, int n, const unsigned* bits, long long first, int count, float* p,
                             int out_cpad, ivf_stream_t stream) {
  const GridStageArgs a{"lin_stage", x, b, C, T, H, W, A_H, A_W, {gt, gh, gw}, first, count, p, out_cpad, stream};
  IVF_PROPAGATE(grid_stage_check(a, bits != nullptr, LIN_MAX_PLAYERS));
  IVF_CHECK_ARG(n > 0 && n <= LIN_MAX_ROWS, "lin_stage: bad row count %d (at most 2^20)", n);
  return grid_stage_launch(a, BitRows{n, lin_words(gt * gh * gw), bits}, (long long)b * (n + 1), "rows");
}

// what ivf_lin_moments, ivf_lin_solve and ivf_lin_fit ask of (b, n, P)
static int lin_dims_check(const char* name, int b, int n, int P, int min_players) {
  IVF_CHECK_ARG(b > 0 && n > 0 && n <= LIN_MAX_ROWS, "%s: bad batch %d or row count %d (at most 2^20)", name, b, n);
  IVF_CHECK_ARG(P >= min_players && P <= LIN_MAX_PLAYERS, "%s: need %d <= P (%d) <= %d players", name, min_players, P,
                LIN_MAX_PLAYERS);
  IVF_CHECK_ARG(((long long)(b + 1) * (P + 1) + 255) / 256 <= 0x7fffffffLL, "%s: too many cells", name);
  return IVF_OK;
}

extern "C" int ivf_lin_moments(const float* scores, const float* score_x, const unsigned* bits, const double* wtab, int b,
                               int n, int P, double* N, double* v, double* Wsum, double* r, double* t, double* wrow,
                               int* ok, ivf_stream_t stream) {
  IVF_CHECK_ARG(scores && score_x && bits && N && v && Wsum && r && t && wrow && ok, "lin_moments: null pointer");
  IVF_PROPAGATE(lin_dims_check("lin_moments", b, n, P, 1));
  hipStream_t s = (hipStream_t)stream;
  const int nw = lin_words(P);
  hipLaunchKernelGGL(lin_wrow_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, bits, wtab, n, nw, wrow);
  hipLaunchKernelGGL(lin_ok_kernel, dim3(b), dim3(256), 0, s, scores, score_x, n, ok);
  hipLaunchKernelGGL(lin_N_kernel, dim3(cdiv(P, 16), cdiv(P, 16)), dim3(256), 0, s, bits, wrow, n, nw, P, N);
  hipLaunchKernelGGL(lin_vr_kernel, dim3(cdiv((long long)(b + 1) * (P + 1), 256)), dim3(256), 0, s, scores, score_x, bits,
                     wrow, b, n, nw, P, v, Wsum, r, t);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" size_t ivf_lin_workspace_bytes(int P) {
  if (P < 1 || P > LIN_MAX_PLAYERS) {
    set_error("lin_workspace_bytes: need 1 <= P (%d) <= %d players", P, LIN_MAX_PLAYERS);
    return 0;
  }
  return LinWork::bytes(P);
}

extern "C" int ivf_lin_solve(int kind, const double* N, const double* v, const double* Wsum, const double* r,
                             const double* t, const float* scores, const float* score_x, int b, int n, int P, double ridge,
                             void* work, float* cells, float* intercept, float* total, int* ok, ivf_stream_t stream) {
  IVF_CHECK_ARG(N && v && Wsum && r && t && scores && score_x && work && cells && intercept && total && ok,
                "lin_solve: null pointer");
  IVF_CHECK_ARG(kind == 0 || kind == 1, "lin_solve: kind must be 0 (kernelshap) or 1 (lime), got %d", kind);
  IVF_PROPAGATE(lin_dims_check("lin_solve", b, n, P, kind == 0 ? 2 : 1));
  IVF_CHECK_ARG(kind == 0 || (ridge >= 0.0 && std::isfinite(ridge)), "lin_solve: ridge must be finite and >= 0, got %g",
                ridge);
  IVF_CHECK_ARG(((uintptr_t)work & 7) == 0, "lin_solve: the workspace is not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int m = kind == 0 ? P - 1 : P;
  const LinWork w(work, P);
  hipLaunchKernelGGL(lin_assemble_kernel, dim3(cdiv((long long)m * m, 256)), dim3(256), 0, s, kind, N, v, Wsum, P, m, ridge,
                     w.A, w.diag0, w.mu, w.flag);
  for (int j0 = 0; j0 < m; j0 += LIN_NB) {
    const int nb = std::min(LIN_NB, m - j0), rest = m - j0 - nb;
    hipLaunchKernelGGL(lin_potrf_kernel, dim3(1), dim3(256), 0, s, w.A, m, j0, nb, w.diag0, w.flag);
    if (rest > 0) {
      hipLaunchKernelGGL(lin_trsm_kernel, dim3(cdiv(rest, 64)), dim3(64), 0, s, w.A, m, j0, nb);
      const int nt = cdiv(rest, LIN_NB);
      hipLaunchKernelGGL(lin_syrk_kernel, dim3(nt, nt), dim3(256), 0, s, w.A, m, j0, nb);
    }
  }
  hipLaunchKernelGGL(lin_subst_kernel, dim3(b), dim3(256), 0, s, kind, w.A, m, N, r, t, Wsum, w.mu, scores, score_x, n, P,
                     w.flag, ok, cells, intercept, total);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_lin_fit(const float* scores, const float* score_x, const unsigned* bits, const double* wrow,
                           const float* cells, const float* intercept, const double* t, const double* Wsum, const int* ok,
                           int b, int n, int P, float* r2, ivf_stream_t stream) {
  IVF_CHECK_ARG(scores && score_x && bits && cells && t && Wsum && ok && r2, "lin_fit: null pointer");
  IVF_PROPAGATE(lin_dims_check("lin_fit", b, n, P, 1));
  hipLaunchKernelGGL(lin_fit_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, scores, score_x, bits, wrow, cells,
                     intercept, t, Wsum, ok, n, lin_words(P), P, r2);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}
