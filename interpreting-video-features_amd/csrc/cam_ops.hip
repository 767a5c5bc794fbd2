// The activation-map family around Grad-CAM: Grad-CAM++ (Chattopadhay et al. 2018), XGrad-CAM (Fu et al.
// 2020), HiResCAM (Draelos & Carin 2020) and LayerCAM (Jiang et al. 2021), from the two buffers a Grad-CAM call
// already holds: the target layer's activations A and the gradient G of the class score with respect to them.
//
//   per clip, p = position, k = channel, s_k = sum_p A[p,k]
//   gradcam++   w_k = sum_p [G > 0] G / (2 + s_k G)                cam[p] = relu(sum_k w_k A[p,k])
//   xgradcam    w_k = (sum_p G A) / s_k, 0 where s_k == 0          cam[p] = relu(sum_k w_k A[p,k])
//   hirescam                                                       cam[p] = relu(sum_k G[p,k] A[p,k])
//   layercam                                                       cam[p] = relu(sum_k relu(G[p,k]) A[p,k])
//
// All of it is HBM-bound.  No atomics, and every sum has one fixed order that depends on (npos, C) alone: a clip's
// weights and maps do not depend on the batch, on the clip's row in it, or on which other kinds the call asked for.
// Kind 'gradcam' runs the kernels of ivf_gradcam_reduce / ivf_clstm_gradcam_reduce themselves.
#include "ivf_common.h"

namespace ivf {

struct bf16s { unsigned short v; };
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ld4(const bf16s* p) {
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const bf16s* p) { return __uint_as_float((unsigned)p->v << 16); }

constexpr int CAM_KINDS = 5;
// positions per workgroup of the per-channel passes: fixed, so the partial sums of a clip never depend on the batch
constexpr int CAM_CHUNK = IVF_CAM_CHUNK;

// slot[k]: row of kind k in the outputs of the call, -1 = not asked for
struct CamSlots {
  int slot[CAM_KINDS];
};

static int cam_slots_from(const int* kinds, int n_kinds, CamSlots* sl, const char* who) {
  IVF_CHECK_ARG(kinds, "%s: null kind list", who);
  IVF_CHECK_ARG(n_kinds >= 1 && n_kinds <= CAM_KINDS, "%s: %d kinds, need 1..%d", who, n_kinds, CAM_KINDS);
  for (int k = 0; k < CAM_KINDS; ++k) sl->slot[k] = -1;
  for (int i = 0; i < n_kinds; ++i) {
    IVF_CHECK_ARG(kinds[i] >= 0 && kinds[i] < CAM_KINDS,
                  "%s: unknown kind %d (0 gradcam, 1 gradcam++, 2 xgradcam, 3 hirescam, 4 layercam)", who, kinds[i]);
    IVF_CHECK_ARG(sl->slot[kinds[i]] < 0, "%s: kind %d listed twice", who, kinds[i]);
    sl->slot[kinds[i]] = i;
  }
  return IVF_OK;
}

// ---------------------------------------------------------------- channels-last [B,npos,C] (the I3D plan)
//
// Per-channel pass over one chunk of CAM_CHUNK positions of one clip.  W channels per thread (4: 16-byte / 8-byte
// loads, C % 4 == 0; 1: any C).  The 256 threads tile (position row, channel column): consecutive threads read
// consecutive channels of one position, R = 256 / columns positions are in flight, a thread walks its positions
// p0 + r, p0 + r + R, ... in order, and row 0 adds the R rows through LDS in row order.
//   PASS 1: part0 = sum A, part1 = sum G A (only if need_ga; grad is not read otherwise)
//   PASS 2: part0 = sum [G > 0] G / (2 + s G), s = the finished sum of PASS 1; reads grad alone
// part{0,1}: [B, nchunks, C].
template <class T, int W, int PASS>
__global__ __launch_bounds__(256) void cam_stats_kernel(const T* __restrict__ feat, const T* __restrict__ grad,
                                                        const float* __restrict__ ssum, float* __restrict__ part0,
                                                        float* __restrict__ part1, int npos, int C, int need_ga) {
  const int chunk = blockIdx.x, b = blockIdx.y, nchunks = gridDim.x;
  const int ncol = C / W;
  const int cw = ncol >= 256 ? 256 : ncol;        // columns per sweep
  const int R = 256 / cw;                         // position rows in flight
  const int r = threadIdx.x / cw, j0 = threadIdx.x % cw;
  const int p0 = chunk * CAM_CHUNK, p1 = min(p0 + CAM_CHUNK, npos);
  __shared__ float sm[2][256][W];
  for (int jb = 0; jb < ncol; jb += cw) {
    const int j = jb + j0;
    const bool on = r < R && j < ncol;
    float a0[W], a1[W], sk[W];
#pragma unroll
    for (int q = 0; q < W; ++q) a0[q] = a1[q] = sk[q] = 0.f;
    if (on) {
      if (PASS == 2) {
#pragma unroll
        for (int q = 0; q < W; ++q) sk[q] = ssum[(size_t)b * C + (size_t)j * W + q];
      }
#pragma unroll 4
      for (int p = p0 + r; p < p1; p += R) {
        const size_t off = ((size_t)b * npos + p) * C + (size_t)j * W;
        float av[W] = {}, gv[W] = {};
        if (W == 4) {
          if (PASS == 1) { float4 v = ld4(feat + off); av[0] = v.x; av[1 % W] = v.y; av[2 % W] = v.z; av[3 % W] = v.w; }
          if (PASS == 2 || need_ga) { float4 v = ld4(grad + off); gv[0] = v.x; gv[1 % W] = v.y; gv[2 % W] = v.z; gv[3 % W] = v.w; }
        } else {
          if (PASS == 1) av[0] = ld1(feat + off);
          if (PASS == 2 || need_ga) gv[0] = ld1(grad + off);
        }
#pragma unroll
        for (int q = 0; q < W; ++q) {
          if (PASS == 1) {
            a0[q] += av[q];
            if (need_ga) a1[q] += gv[q] * av[q];
          } else {
            // the closed form for an exponential score, G^2 / (2 G^2 + s G^3), with G^2 cancelled: G^3 of a
            // near-uniform softmax is an fp32 denormal
            const float al = gv[q] > 0.f ? 1.f / (2.f + sk[q] * gv[q]) : 0.f;
            a0[q] += al * gv[q];
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < W; ++q) {
      sm[0][threadIdx.x][q] = a0[q];
      sm[1][threadIdx.x][q] = a1[q];
    }
    __syncthreads();
    if (on && r == 0) {
#pragma unroll
      for (int q = 0; q < W; ++q) {
        float t0 = a0[q], t1 = a1[q];
        for (int rr = 1; rr < R; ++rr) {
          t0 += sm[0][rr * cw + j0][q];
          t1 += sm[1][rr * cw + j0][q];
        }
        const size_t o = ((size_t)b * nchunks + chunk) * C + (size_t)j * W + q;
        part0[o] = t0;
        if (PASS == 1 && need_ga) part1[o] = t1;
      }
    }
    __syncthreads();
  }
}

// Adds the chunks of a clip in index order, one thread per (clip, channel).
//   PASS 1: ssum = s_k; if need_ga: w_x = sum G A / s_k, 0 where s_k == 0, to wbuf and (optional) wout
//   PASS 2: w_pp to wbuf and (optional) wout
template <int PASS>
__global__ __launch_bounds__(256) void cam_finish_kernel(const float* __restrict__ part0, const float* __restrict__ part1,
                                                         float* __restrict__ ssum, float* __restrict__ wbuf,
                                                         float* __restrict__ wout, int nchunks, int C, int B,
                                                         int need_ga) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i % C;
  float t0 = 0.f, t1 = 0.f;
  for (int k = 0; k < nchunks; ++k) {
    const size_t o = ((size_t)b * nchunks + k) * C + c;
    t0 += part0[o];
    if (PASS == 1 && need_ga) t1 += part1[o];
  }
  if (PASS == 1) {
    ssum[i] = t0;
    if (need_ga) {
      const float w = t0 == 0.f ? 0.f : t1 / t0;
      wbuf[i] = w;
      if (wout) wout[i] = w;
    }
  } else {
    wbuf[i] = t0;
    if (wout) wout[i] = t0;
  }
}

// The maps of kinds 1..4 in one sweep: one wave per position, lanes striding over channels (W = 4: four channels
// per lane and step).  feat is read once, grad once and only if HiResCAM or LayerCAM is asked for; every kind has
// its own accumulator, so a kind's map does not depend on the others.  cam: [n_kinds, B, npos].
template <class T, int W>
__global__ __launch_bounds__(256) void cam_maps_kernel(const T* __restrict__ feat, const T* __restrict__ grad,
                                                       const float* __restrict__ w_pp, const float* __restrict__ w_x,
                                                       float* __restrict__ cam, CamSlots sl, int npos, int C, int B) {
  const long gw = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (gw >= (long)B * npos) return;
  const int b = (int)(gw / npos);
  const T* f = feat + (size_t)gw * C;
  const T* g = grad + (size_t)gw * C;
  const float* wp = w_pp + (size_t)b * C;
  const float* wx = w_x + (size_t)b * C;
  const bool k1 = sl.slot[1] >= 0, k2 = sl.slot[2] >= 0, k3 = sl.slot[3] >= 0, k4 = sl.slot[4] >= 0;
  float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
  for (int c = lane * W; c < C; c += 64 * W) {
    float av[W] = {}, gv[W] = {};
    if (W == 4) {
      float4 v = ld4(f + c);
      av[0] = v.x; av[1 % W] = v.y; av[2 % W] = v.z; av[3 % W] = v.w;
      if (k3 || k4) { float4 u = ld4(g + c); gv[0] = u.x; gv[1 % W] = u.y; gv[2 % W] = u.z; gv[3 % W] = u.w; }
    } else {
      av[0] = ld1(f + c);
      if (k3 || k4) gv[0] = ld1(g + c);
    }
#pragma unroll
    for (int q = 0; q < W; ++q) {
      if (k1) s1 += wp[c + q] * av[q];
      if (k2) s2 += wx[c + q] * av[q];
      if (k3) s3 += gv[q] * av[q];
      if (k4) s4 += fmaxf(gv[q], 0.f) * av[q];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_down(s1, o, 64);
    s2 += __shfl_down(s2, o, 64);
    s3 += __shfl_down(s3, o, 64);
    s4 += __shfl_down(s4, o, 64);
  }
  if (lane == 0) {
    const size_t n = (size_t)B * npos;
    if (k1) cam[sl.slot[1] * n + gw] = fmaxf(s1, 0.f);
    if (k2) cam[sl.slot[2] * n + gw] = fmaxf(s2, 0.f);
    if (k3) cam[sl.slot[3] * n + gw] = fmaxf(s3, 0.f);
    if (k4) cam[sl.slot[4] * n + gw] = fmaxf(s4, 0.f);
  }
}

// workspace, in floats: ssum [B,C] | w of kinds 0, 1, 2 [3,B,C] | part0, part1 [2,B,nchunks,C]
struct CamWs {
  float *ssum, *w0, *w_pp, *w_x, *part0, *part1;
};
static inline int cam_chunks(int npos) { return (npos + CAM_CHUNK - 1) / CAM_CHUNK; }
static CamWs cam_carve(void* ws, int B, int npos, int C) {
  const size_t bc = (size_t)B * C, pc = bc * cam_chunks(npos);
  float* f = (float*)ws;
  return CamWs{f, f + bc, f + 2 * bc, f + 3 * bc, f + 4 * bc, f + 4 * bc + pc};
}

template <class T, int W>
static int cam_reduce_launch(const T* feat, const T* grad, const CamSlots& sl, float* weights, float* cam,
                             const CamWs& w, int B, int npos, int C, hipStream_t s) {
  const size_t bc = (size_t)B * C;
  const dim3 grid(cam_chunks(npos), B);
  const int need_ga = sl.slot[IVF_CAM_XGRAD] >= 0;
  auto wrow = [&](int kind) { return weights ? weights + sl.slot[kind] * bc : (float*)nullptr; };
  if (sl.slot[IVF_CAM_PP] >= 0 || need_ga) {
    hipLaunchKernelGGL((cam_stats_kernel<T, W, 1>), grid, dim3(256), 0, s, feat, grad, (const float*)nullptr, w.part0,
                       w.part1, npos, C, need_ga);
    IVF_CHECK_LAUNCH();
    hipLaunchKernelGGL((cam_finish_kernel<1>), dim3(cdiv(bc, 256)), dim3(256), 0, s, w.part0, w.part1, w.ssum, w.w_x,
                       need_ga ? wrow(IVF_CAM_XGRAD) : (float*)nullptr, (int)grid.x, C, B, need_ga);
    IVF_CHECK_LAUNCH();
  }
  if (sl.slot[IVF_CAM_PP] >= 0) {
    hipLaunchKernelGGL((cam_stats_kernel<T, W, 2>), grid, dim3(256), 0, s, feat, grad, w.ssum, w.part0, w.part1, npos,
                       C, 0);
    IVF_CHECK_LAUNCH();
    hipLaunchKernelGGL((cam_finish_kernel<2>), dim3(cdiv(bc, 256)), dim3(256), 0, s, w.part0, w.part1, w.ssum, w.w_pp,
                       wrow(IVF_CAM_PP), (int)grid.x, C, B, 0);
    IVF_CHECK_LAUNCH();
  }
  bool maps = false;
  for (int k = 1; k < CAM_KINDS; ++k) maps = maps || sl.slot[k] >= 0;
  if (maps) {
    hipLaunchKernelGGL((cam_maps_kernel<T, W>), dim3(cdiv((long long)B * npos * 64, 256)), dim3(256), 0, s, feat, grad,
                       w.w_pp, w.w_x, cam, sl, npos, C, B);
    IVF_CHECK_LAUNCH();
  }
  return IVF_OK;
}

int cam_reduce(const void* feat, const void* grad, bool bf16, int n_kinds, const int* kinds, float* weights,
               float* cam, void* ws, int B, int npos, int C, hipStream_t s) {
  IVF_CHECK_ARG(feat && grad && cam && ws, "cam_reduce: null pointer");
  IVF_CHECK_ARG(B > 0 && B <= 65535 && npos > 0 && C > 0, "cam_reduce: bad dims");
  IVF_CHECK_ARG((long long)B * npos * 64 / 256 < 2147483647LL, "cam_reduce: too many positions for one launch");
  CamSlots sl;
  IVF_PROPAGATE(cam_slots_from(kinds, n_kinds, &sl, "cam_reduce"));
  const CamWs w = cam_carve(ws, B, npos, C);
  const size_t bc = (size_t)B * C, bp = (size_t)B * npos;
  if (sl.slot[IVF_CAM_GRADCAM] >= 0) {     // the kernels of ivf_gradcam_reduce themselves: bit-equal to it
    IVF_PROPAGATE(gradcam_reduce(feat, grad, bf16, w.w0, cam + sl.slot[IVF_CAM_GRADCAM] * bp, B, npos, C, s));
    if (weights)
      IVF_CHECK_HIP(hipMemcpyAsync(weights + sl.slot[IVF_CAM_GRADCAM] * bc, w.w0, bc * 4, hipMemcpyDeviceToDevice, s));
  }
  if (weights)
    for (int k : {IVF_CAM_HIRES, IVF_CAM_LAYER})
      if (sl.slot[k] >= 0) IVF_CHECK_HIP(hipMemsetAsync(weights + sl.slot[k] * bc, 0, bc * 4, s));
  if (C % 4 == 0) {
    if (bf16) return cam_reduce_launch<bf16s, 4>((const bf16s*)feat, (const bf16s*)grad, sl, weights, cam, w, B, npos, C, s);
    return cam_reduce_launch<float, 4>((const float*)feat, (const float*)grad, sl, weights, cam, w, B, npos, C, s);
  }
  if (bf16) return cam_reduce_launch<bf16s, 1>((const bf16s*)feat, (const bf16s*)grad, sl, weights, cam, w, B, npos, C, s);
  return cam_reduce_launch<float, 1>((const float*)feat, (const float*)grad, sl, weights, cam, w, B, npos, C, s);
}

// ---------------------------------------------------------------- [B,T,hid,plane] fp32 (the ConvLSTM plan)
struct CamStepList {
  int n;
  int s[64];
};

// block-wide sum of doubles in a fixed order: lanes by shuffles, the 4 waves through LDS, added in wave order;
// every thread gets the total
__device__ __forceinline__ double block_sum256(double v, double* part) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();          // `part` may still be read from the previous call
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((part[0] + part[1]) + part[2]) + part[3];
}

// One workgroup per clip.  hid is small and a clip's maps are a few thousand positions: the per-channel sums stay in
// LDS, and a thread owns map pixels and walks the channels in order.  Partial sums are fp64 as in
// clstm_cam_weights_kernel (signed values that largely cancel).  weights: [n_kinds,B,hid] or null; cam:
// [n_kinds,B,n_steps,plane]; kind 0 is not handled here.
__global__ __launch_bounds__(256) void clstm_cam_family_kernel(const float* __restrict__ feat,
                                                               const float* __restrict__ grad, CamStepList st,
                                                               CamSlots sl, float* __restrict__ weights,
                                                               float* __restrict__ cam, int T, int hid, int plane) {
  const int b = blockIdx.x, B = gridDim.x;
  __shared__ double part[4];
  __shared__ float w_pp[IVF_CAM_MAX_HID], w_x[IVF_CAM_MAX_HID];
  const bool k1 = sl.slot[1] >= 0, k2 = sl.slot[2] >= 0, k3 = sl.slot[3] >= 0, k4 = sl.slot[4] >= 0;
  if (k1 || k2)
    for (int c = 0; c < hid; ++c) {
      double sa = 0.0, sga = 0.0;
      for (int e = 0; e < st.n; ++e) {
        const long o = (((long)b * T + st.s[e]) * hid + c) * plane;
        for (int i = threadIdx.x; i < plane; i += 256) {
          const float a = feat[o + i];
          sa += (double)a;
          if (k2) sga += (double)(grad[o + i] * a);
        }
      }
      sa = block_sum256(sa, part);
      if (k2) sga = block_sum256(sga, part);
      const float s = (float)sa;
      if (k1) {
        double acc = 0.0;
        for (int e = 0; e < st.n; ++e) {
          const long o = (((long)b * T + st.s[e]) * hid + c) * plane;
          for (int i = threadIdx.x; i < plane; i += 256) {
            const float g = grad[o + i];
            const float al = g > 0.f ? 1.f / (2.f + s * g) : 0.f;
            acc += (double)(al * g);
          }
        }
        acc = block_sum256(acc, part);
        if (threadIdx.x == 0) w_pp[c] = (float)acc;
      }
      if (k2 && threadIdx.x == 0) w_x[c] = s == 0.f ? 0.f : (float)sga / s;
    }
  __syncthreads();
  if (weights && threadIdx.x < hid) {
    const int c = threadIdx.x;
    if (k1) weights[((long)sl.slot[1] * B + b) * hid + c] = w_pp[c];
    if (k2) weights[((long)sl.slot[2] * B + b) * hid + c] = w_x[c];
    if (k3) weights[((long)sl.slot[3] * B + b) * hid + c] = 0.f;
    if (k4) weights[((long)sl.slot[4] * B + b) * hid + c] = 0.f;
  }
  const long nmap = (long)st.n * plane;
  for (long m = threadIdx.x; m < nmap; m += 256) {
    const int e = (int)(m / plane), i = (int)(m % plane);
    const long o = ((long)b * T + st.s[e]) * hid * plane + i;
    float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
    for (int c = 0; c < hid; ++c) {
      const float a = feat[o + (long)c * plane];
      if (k1) s1 += w_pp[c] * a;
      if (k2) s2 += w_x[c] * a;
      if (k3 || k4) {
        const float g = grad[o + (long)c * plane];
        if (k3) s3 += g * a;
        if (k4) s4 += fmaxf(g, 0.f) * a;
      }
    }
    const long q = (long)b * nmap + m, n = (long)B * nmap;
    if (k1) cam[sl.slot[1] * n + q] = fmaxf(s1, 0.f);
    if (k2) cam[sl.slot[2] * n + q] = fmaxf(s2, 0.f);
    if (k3) cam[sl.slot[3] * n + q] = fmaxf(s3, 0.f);
    if (k4) cam[sl.slot[4] * n + q] = fmaxf(s4, 0.f);
  }
}

}  // namespace ivf

using namespace ivf;

extern "C" size_t ivf_cam_ws_bytes(int B, int npos, int C) {
  if (B <= 0 || npos <= 0 || C <= 0) return 0;
  return align_up(((size_t)4 + 2 * (size_t)cam_chunks(npos)) * B * C * sizeof(float), 256);
}

extern "C" int ivf_cam_reduce(const float* feat, const float* grad, int n_kinds, const int* kinds_host, float* weights,
                              float* cam, void* ws, int B, int npos, int C, ivf_stream_t stream) {
  return cam_reduce(feat, grad, false, n_kinds, kinds_host, weights, cam, ws, B, npos, C, (hipStream_t)stream);
}

extern "C" int ivf_cam_reduce_bf16(const void* feat, const void* grad, int n_kinds, const int* kinds_host,
                                   float* weights, float* cam, void* ws, int B, int npos, int C, ivf_stream_t stream) {
  return cam_reduce(feat, grad, true, n_kinds, kinds_host, weights, cam, ws, B, npos, C, (hipStream_t)stream);
}

extern "C" int ivf_clstm_cam_reduce(const float* feat, const float* grad, const int* steps_host, int n_steps,
                                    int n_kinds, const int* kinds_host, float* weights, float* cam, int B, int T,
                                    int hid, int plane, ivf_stream_t stream) {
  IVF_CHECK_ARG(feat && grad && cam, "clstm_cam_reduce: null pointer");
  IVF_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && hid > 0 && hid <= IVF_CAM_MAX_HID && plane > 0,
                "clstm_cam_reduce: bad dims (hid 1..%d)", IVF_CAM_MAX_HID);
  IVF_CHECK_ARG(n_steps > 0 && n_steps <= 64, "clstm_cam_reduce: 1..64 steps");
  CamStepList st;
  st.n = n_steps;
  for (int e = 0; e < n_steps; ++e) {
    st.s[e] = steps_host ? steps_host[e] : e;
    IVF_CHECK_ARG(st.s[e] >= 0 && st.s[e] < T, "clstm_cam_reduce: step %d outside [0,%d)", st.s[e], T);
  }
  CamSlots sl;
  IVF_PROPAGATE(cam_slots_from(kinds_host, n_kinds, &sl, "clstm_cam_reduce"));
  hipStream_t s = (hipStream_t)stream;
  const size_t bh = (size_t)B * hid, bm = (size_t)B * n_steps * plane;
  if (sl.slot[IVF_CAM_GRADCAM] >= 0) {     // the kernels of ivf_clstm_gradcam_reduce themselves: bit-equal to it
    // their map kernel reads the weights from global memory and this entry has no workspace: the caller's row it is
    IVF_CHECK_ARG(weights, "clstm_cam_reduce: kind 0 (gradcam) needs the weights output");
    IVF_PROPAGATE(ivf_clstm_gradcam_reduce(feat, grad, st.s, n_steps, weights + sl.slot[IVF_CAM_GRADCAM] * bh,
                                           cam + sl.slot[IVF_CAM_GRADCAM] * bm, B, T, hid, plane, stream));
  }
  bool rest = false;
  for (int k = 1; k < CAM_KINDS; ++k) rest = rest || sl.slot[k] >= 0;
  if (rest) {
    hipLaunchKernelGGL(clstm_cam_family_kernel, dim3(B), dim3(256), 0, s, feat, grad, st, sl, weights, cam, T, hid,
                       plane);
    IVF_CHECK_LAUNCH();
  }
  return IVF_OK;
}
