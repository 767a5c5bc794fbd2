// Shared host-side helpers for libivf_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include <type_traits>

#include "../../include/ivf_hip.h"

namespace ivf {

// most frames of a mask: the freeze backward kernels keep a pixel's frames in registers, the regularisers a row in
// a thread's private arrays
constexpr int MAX_T = 64;

void set_error(const char* fmt, ...);

// launch profiler (ivf_common.hip)
void prof_set_iteration(int it);
void prof_set_flops(double algorithmic_flops);
void prof_set_site(int site);   // launch site of the next sampled launches (2 * op index + direction), -1 none
bool prof_begin(hipStream_t s, int variant);
void prof_end(hipStream_t s);
void prof_name(int variant, const char* fmt, ...);   // kernel name of a profiler class (first call wins)

// freeze scan (mask_ops.hip) behind ivf_freeze_fwd and ivf_stfreeze_fwd, arguments checked by them: `mask` holds one
// value per frame ([B,T], or [T] with mask_per_clip == 0) or, with pixel_mask, one per frame and pixel ([B,T,HW])
int freeze_fwd(const float* x, const float* mask, bool pixel_mask, float* p, int B, int C, int T, int HW,
               int mask_per_clip, int out_cpad, hipStream_t s);

// one-blob search (mask_ops.hip): scores[first + j] = probs[j][target[(first + j) / n]] for the `count` rows of a chunk
int blob_pick(const float* probs, const int* target, int K, int n, long long first, int count, float* scores,
              hipStream_t s);

// Integrated Gradients (ig_ops.hip): rowt[g] = target[g / K] for the b * K rows of the (clip, node) list
int ig_row_targets(const int* target, int b, int K, int* rowt, hipStream_t s);

// index k of the canonical one-blob order (length ascending, then start) on an axis of T positions -> (start, length);
// the three axes of the one-box search (stmask_ops.hip) decode with it as well
__device__ __forceinline__ void blob_decode(int k, int T, int* a, int* L) {
  int l = 1;
  while (k >= T - l + 1) {
    k -= T - l + 1;
    ++l;
  }
  *a = k;
  *L = l;
}

// classification head and Grad-CAM reduction (pool_head.hip) on activations / gradients stored as fp32, or as bf16 when
// `bf16` is set: what ivf_head_fwd{,_bf16}, ivf_head_bwd{,_bf16} and ivf_gradcam_reduce{,_bf16} do, storage type at run time
int head_fwd(const void* feat, bool bf16, const float* w, const float* bias, float* pooled, float* logits, float* probs,
             int B, int npos, int C, int K, int softmax, hipStream_t s);
int head_bwd(const void* feat, bool bf16, const float* w, const float* probs, const int* target, const float* dout,
             float* score, float* dpooled, void* dfeat, int B, int npos, int C, int K, int softmax, int gate_relu,
             hipStream_t s);
int gradcam_reduce(const void* feat, const void* grad, bool bf16, float* weights, float* cam, int B, int npos, int C,
                   hipStream_t s);
// the Grad-CAM family (cam_ops.hip) in either storage: what ivf_cam_reduce{,_bf16} do
int cam_reduce(const void* feat, const void* grad, bool bf16, int n_kinds, const int* kinds, float* weights,
               float* cam, void* ws, int B, int npos, int C, hipStream_t s);

#define IVF_CHECK_ARG(cond, ...)                 \
  do {                                           \
    if (!(cond)) {                               \
      ::ivf::set_error(__VA_ARGS__);             \
      return IVF_ERR_BAD_ARG;                    \
    }                                            \
  } while (0)

#define IVF_CHECK_HIP(expr)                                                        \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) {                                                        \
      ::ivf::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),      \
                       __FILE__, __LINE__);                                        \
      return IVF_ERR_HIP;                                                          \
    }                                                                              \
  } while (0)

#define IVF_CHECK_LAUNCH() IVF_CHECK_HIP(hipGetLastError())

#define IVF_PROPAGATE(expr)      \
  do {                           \
    int rc_ = (expr);            \
    if (rc_ != IVF_OK) return rc_; \
  } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize once per (kernel, device): `done` is the call site's static flag array
struct LdsAttrOnce { bool done[32] = {}; };
static inline int raise_lds_limit(const void* kernel, int bytes, LdsAttrOnce& once) {
  int dev = 0;
  IVF_CHECK_HIP(hipGetDevice(&dev));
  if (dev >= 0 && dev < 32 && once.done[dev]) return IVF_OK;
  IVF_CHECK_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  if (dev >= 0 && dev < 32) once.done[dev] = true;
  return IVF_OK;
}

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// blocks of a grid-stride launch over `total` elements: at least 1, at most `cap`
static inline int grid_for(size_t total, int block = 256, int cap = 4096) {
  size_t g = (total + block - 1) / block;
  return (int)(g > (size_t)cap ? cap : (g ? g : 1));
}

// Frame count as a compile-time constant, in the manner of with_const_1to4 (convlstm.hip): f(integral_constant<int, TT>).
// exact: TT == T for the two clip lengths whose forward scans are unrolled, else 0 (the run-time loop, any T).
template <class F>
static inline void with_frames_exact(int T, F&& f) {
  if (T == 16) f(std::integral_constant<int, 16>{});
  else if (T == 32) f(std::integral_constant<int, 32>{});
  else f(std::integral_constant<int, 0>{});
}
// upto: the smallest TT of 16, 32, MAX_T with T <= TT (register arrays of the backward scans)
template <class F>
static inline void with_frames_upto(int T, F&& f) {
  if (T <= 16) f(std::integral_constant<int, 16>{});
  else if (T <= 32) f(std::integral_constant<int, 32>{});
  else f(std::integral_constant<int, MAX_T>{});
}

// torch.optim.Adam's bias corrections of step `step`, in double as torch computes them
static inline void adam_coeffs(int step, float lr, float b1, float b2, float* step_size, float* inv_sqrt_bc2) {
  double bc1 = 1.0 - pow((double)b1, step);
  double bc2 = 1.0 - pow((double)b2, step);
  *step_size = (float)((double)lr / bc1);
  *inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
}

// TF-'same' front padding along one dim (reference I3D_doubled.py:9-13, 29-34).
static inline void same_pad(int n, int k, int s, int* front, int* back) {
  int p = (n % s == 0) ? (k - s) : (k - (n % s));
  if (p < 0) p = 0;
  *front = p / 2;
  *back = p - p / 2;
}
static inline int same_out(int n, int k, int s) {
  int f, b;
  same_pad(n, k, s, &f, &b);
  return (n + f + b - k) / s + 1;
}

// Workgroups are dealt round-robin over the 8 XCDs (each with its own L2): hand every XCD a contiguous range of
// tiles, so that tiles sharing input rows share an L2 (bijective on [0, nwg)).
__device__ __forceinline__ int xcd_remap(int id, int nwg) {
  // Blocks are dealt round-robin over 8 XCDs; give each XCD a contiguous range of
  // tiles so blocks sharing an A panel share an L2 (bijective form).
  int q = nwg >> 3, r = nwg & 7;
  int xcd = id & 7, pos = id >> 3;
  int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + pos;
}

}  // namespace ivf
