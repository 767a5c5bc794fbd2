// RISE random-mask saliency for video (Petsiuk et al. 2018), an EXTENSION with no counterpart in the reference
// (DESIGN 14): n random coarse masks per clip, one forward each, a cell's importance = the mean score drop over the
// masks that froze it.
//
// The mask family is integer-exact and the same for every clip.  A mask lives on a grid (gt, gh, gw), and mask k freezes
// cell c iff
//   u(seed, k, c) = grid_hash(grid_key(seed, k), c) < thresh                                  (uint32, grid_stage.h)
// Nothing stores the masks: staging and reduction regenerate the bits.  The staging kernels and their scan are the
// shared ones of grid_stage.h; this file gives them the rows.
#include "grid_stage.h"

namespace ivf {

// row r of the flattened (clip, mask) list: cell c frozen iff its hash is below the threshold
struct RiseRows {
  int n;                 // masks per clip
  unsigned seed, thresh;
  struct Cells {
    int clip;
    unsigned key, thresh;
    __device__ __forceinline__ bool frozen(int c) const { return grid_hash(key, c) < thresh; }
  };
  __device__ __forceinline__ Cells cells(long long r, int) const { return {(int)(r / n), grid_key(seed, (int)(r % n)), thresh}; }
  __device__ __forceinline__ bool bit(int k, int c) const { return grid_hash(grid_key(seed, k), c) < thresh; }
};

// ---------------------------------------------------------------- explicit bits
__global__ __launch_bounds__(256) void rise_masks_kernel(RiseRows q, int cells, int first_k, int count,
                                                         float* __restrict__ S) {
  const size_t e = blockIdx.x * (size_t)256 + threadIdx.x;
  if (e >= (size_t)count * cells) return;
  const int r = (int)(e / cells), c = (int)(e - (size_t)r * cells);
  S[e] = q.bit(first_k + r, c) ? 1.f : 0.f;
}

// ---------------------------------------------------------------- reduction
// One thread per (clip, cell) walks the masks in ascending k, d_k = orig - s_k: cells = sum over the masks that froze
// the cell / their count, a NaN score neither summed nor counted (as ivf_box_drop), NaN where nothing is counted.  The
// thread of a clip's cell 0 also walks all of the clip's masks for mean_drop.  Plain fp32 adds in a fixed order, no
// atomics, the bits regenerated from the hash: a clip's numbers do not depend on the batch.
__global__ __launch_bounds__(256) void rise_reduce_kernel(const float* __restrict__ scores, const float* __restrict__ orig,
                                                          int B, int cells, RiseRows q, float* __restrict__ cells_out,
                                                          int* __restrict__ count_out, float* __restrict__ mean_drop) {
  const size_t e = blockIdx.x * (size_t)256 + threadIdx.x;
  if (e >= (size_t)B * cells) return;
  const int b = (int)(e / cells), c = (int)(e - (size_t)b * cells);
  const float* s = scores + (size_t)b * q.n;
  const float o = orig[b];
  float sum = 0.f, all = 0.f;
  int cnt = 0, nall = 0;
  for (int k = 0; k < q.n; ++k) {
    const float v = s[k];
    if (v != v) continue;
    const float d = o - v;
    all += d;
    ++nall;
    if (q.bit(k, c)) {
      sum += d;
      ++cnt;
    }
  }
  cells_out[e] = cnt ? sum / (float)cnt : __builtin_nanf("");
  count_out[e] = cnt;
  if (c == 0) mean_drop[b] = nall ? all / (float)nall : __builtin_nanf("");
}

}  // namespace ivf

using namespace ivf;

extern "C" int ivf_rise_masks(unsigned seed, unsigned thresh, int first_k, int count, int gt, int gh, int gw, float* S,
                              ivf_stream_t stream) {
  IVF_CHECK_ARG(S, "rise_masks: null pointer");
  IVF_PROPAGATE(grid_check("rise_masks", MAX_T, gt, gh, gw));     // the clip length is not this entry's: gt <= MAX_T
  IVF_CHECK_ARG(thresh != 0, "rise_masks: thresh must be > 0 (thresh = floor(p 2^32), 0 < p < 1)");
  IVF_CHECK_ARG(first_k >= 0 && count > 0 && (long long)first_k + count <= 0x7fffffffLL,
                "rise_masks: masks [%d, %lld) outside 0 .. 2^31 - 1", first_k, (long long)first_k + count);
  const long long total = (long long)count * gt * gh * gw;
  IVF_CHECK_ARG((total + 255) / 256 <= 0x7fffffffLL, "rise_masks: too many cells");
  hipLaunchKernelGGL(rise_masks_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     RiseRows{0, seed, thresh}, gt * gh * gw, first_k, count, S);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}

extern "C" int ivf_rise_stage(const float* x, int b, int C, int T, int H, int W, const float* A_H, const float* A_W, int gt,
                              int gh, int gw, int n, unsigned seed, unsigned thresh, long long first, int count, float* p,
                              int out_cpad, ivf_stream_t stream) {
  const GridStageArgs a{"rise_stage", x, b, C, T, H, W, A_H, A_W, {gt, gh, gw}, first, count, p, out_cpad, stream};
  IVF_PROPAGATE(grid_stage_check(a, true, 0));
  IVF_CHECK_ARG(thresh != 0, "rise_stage: thresh must be > 0 (thresh = floor(p 2^32), 0 < p < 1)");
  IVF_CHECK_ARG(n > 0, "rise_stage: bad mask count %d", n);
  return grid_stage_launch(a, RiseRows{n, seed, thresh}, (long long)b * n, "masks");
}

extern "C" int ivf_rise_reduce(const float* scores, const float* orig, int b, int n, unsigned seed, unsigned thresh, int gt,
                               int gh, int gw, float* cells, int* count, float* mean_drop, ivf_stream_t stream) {
  IVF_CHECK_ARG(scores && orig && cells && count && mean_drop, "rise_reduce: null pointer");
  IVF_CHECK_ARG(b > 0 && n > 0, "rise_reduce: bad batch %d or mask count %d", b, n);
  IVF_PROPAGATE(grid_check("rise_reduce", MAX_T, gt, gh, gw));
  IVF_CHECK_ARG(thresh != 0, "rise_reduce: thresh must be > 0 (thresh = floor(p 2^32), 0 < p < 1)");
  const long long total = (long long)b * gt * gh * gw;
  IVF_CHECK_ARG((total + 255) / 256 <= 0x7fffffffLL, "rise_reduce: too many cells");
  hipLaunchKernelGGL(rise_reduce_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, scores, orig, b,
                     gt * gh * gw, RiseRows{n, seed, thresh}, cells, count, mean_drop);
  IVF_CHECK_LAUNCH();
  return IVF_OK;
}
