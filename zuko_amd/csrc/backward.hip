// zuko_amd — backward (vector-Jacobian product) kernels of the univariate transforms, the base
// density and the activations: SURVEY 8(f) rank 1.  The reference has no backward code of its own —
// `loss.backward()` runs PyTorch autograd through every ATen op of the forward
// (zuko/transforms.py:480-490, 554-567 for the spline; :436-446 affine) — so these kernels are the
// fused adjoints of those op sequences.
//
// Spline: given gy[N, D] and gl (the gradient w.r.t. log|det J|, per row when the forward reduced over
// features), produce gx[N, D] and g_phi[N, D, 3K-1] for the PACKED parameter layout.  Per element the
// forward is recomputed from phi (same device functions as the forward kernels), the local map
//   (x, x0, x1, y0, y1, d0, d1) -> (y, ladj)
// is differentiated with 7-wide forward-mode dual numbers (no hand-derived formulas to get wrong), and
// the adjoint is pushed back through bin gather -> cumsum -> softmax -> softclip / exp by hand (those
// are sparse: only the two knots of the active bin receive gradient).
// Data movement mirrors the forward kernel: a wave owns 64 consecutive elements, phi comes in and
// g_phi goes out through a wave-private LDS image with 16-byte global accesses.
#include "zk_stage.h"
#include "zk_univariate_bwd.h"

namespace zk {

struct BwdArgs {
  int64_t N, D;
  const float* x;
  const float* phi;   // [N, D, total] packed
  const float* gy;    // [N, D]
  const float* gl;    // [N] (reduced) or [N, D]
  int gl_reduced;
  float* gx;          // [N, D]
  float* gphi;        // [N, D, total]
  float bound, ls;
  int64_t iters;
};

extern __shared__ __attribute__((aligned(16))) float bw_lds[];

// The frame of the packed adjoints: a wave owns 64 consecutive elements; their parameters come in through the wave-private LDS image, `elem(slot, x,
// gy, gl)` replaces an element's `total` parameters in the image by their gradients (in place: a lane's own words) and returns gx, and the image goes
// out as g_phi.  `total` is a count (zk_univariate.h): Fixed for the kinds whose element lives in registers, Dyn for a run-time size.  Requires phi and
// gphi of the same alignment modulo 16 bytes; any N, D.
template <class C, typename Elem> __device__ __forceinline__ void uni_backward_frame(const BwdArgs& a, C total_count, Elem elem) {
  const int total = total_count;
  const int per_wave = 64 * total + 8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* wsh = bw_lds + wave * per_wave;
  const int64_t total_elems = a.N * a.D;
  const int64_t wt0 = ((int64_t)blockIdx.x * 4 + wave) * a.iters;
  for (int64_t it = 0; it < a.iters; ++it) {
    const int64_t e0 = (wt0 + it) * 64;
    if (e0 >= total_elems) break;  // wave-uniform
    const int64_t cnt = (total_elems - e0) < 64 ? (total_elems - e0) : 64;
    const float* src = a.phi + e0 * total;
    const int shift = (int)(((uintptr_t)src / 4) % 4);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    stage_contiguous<float>(src, wsh, cnt * total, lane);  // (alignment-preserving image, as the forward kernel)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if (lane < cnt) {
      const int64_t e = e0 + lane;
      const float glv = a.gl ? (a.gl_reduced ? a.gl[e / a.D] : a.gl[e]) : 0.f;
      const float gyv = a.gy ? a.gy[e] : 0.f;
      a.gx[e] = elem(wsh + shift + lane * total, a.x[e], gyv, glv);
    }
    // g_phi out through the same LDS image (same shift: gphi has the alignment of phi by contract)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    unstage_contiguous<float>(wsh, shift, a.gphi + e0 * total, cnt * total, lane);
  }
}

// KIND 0: affine (total 2), 1: RQS with K bins.
template <int KIND, int K> __global__ __launch_bounds__(256) void uni_backward_kernel(BwdArgs a) {
  constexpr int TOTAL = KIND == 0 ? 2 : 3 * K - 1;
  uni_backward_frame(a, Fixed<TOTAL>{}, [&](float* slot, float x, float gyv, float glv) {
    float p[TOTAL], g[TOTAL];
    float gxv = 0.f;
#pragma unroll
    for (int i = 0; i < TOTAL; ++i) p[i] = slot[i];
    if (KIND == 0) affine_backward_element(p, x, gyv, glv, a.ls, gxv, g);
    else rqs_backward_element<K>(p, x, gyv, glv, a.bound, a.ls, gxv, g);
#pragma unroll
    for (int i = 0; i < TOTAL; ++i) slot[i] = g[i];
    return gxv;
  });
}

// Gaussianization with a run-time component count K <= ZK_GAUSS_KMAX_BWD: phi = [b(K) | a(K)] per element
__global__ __launch_bounds__(256) void gauss_backward_kernel(BwdArgs a, int K) {
  uni_backward_frame(a, Dyn<2 * ZK_GAUSS_KMAX_BWD>{2 * K}, [&](float* slot, float x, float gyv, float glv) { return gauss_backward_element(K, slot, x, gyv, glv); });
}

// Gaussianization with ONE [D, 2K] parameter table shared by all rows (the unconditional GF): gx as above, and the table's gradient summed over the
// rows inside the kernel instead of written per row.  Geometry: block (c, t) covers the rows of chunk c and the features d0 = 64 t ..
// d0 + dw - 1, dw = min(64, D - d0); lane l of a wave stays on feature d0 + l % dw and walks the rows r + l / dw (64 / dw rows per wave and pass,
// lanes beyond (64 / dw) dw idle), so x / gy / gx are read and written along the feature axis and a lane's [2K] running sums are its own LDS words.
// LDS: acc[2K][256] (component-major: the 64 lanes of a wave touch 64 consecutive banks) | par[2K][64] (the tile's parameters transposed: lanes of
// consecutive features read consecutive banks, lanes of one feature the same word).  At the end of the chunk the lanes of one feature are added in
// the fixed order (wave, row slot) and the tile's [dw, 2K] partial goes to work[c]; gauss_shared_reduce_kernel adds the chunks.  No atomics.
struct GaussSharedArgs {
  int64_t N, D;
  const float *x, *phi, *gy, *gl;
  int gl_reduced, K;
  float *gx, *work;
  int64_t passes;  // of pass_rows rows each, split evenly over gridDim.x chunks
  int pass_rows;
};

// the partition, a function of (N, D, K) alone: a pass is what one block covers of a full feature tile in one step (4 waves x 64 / min(64, D) rows); a
// chunk has eight passes until there are GAUSS_SHARED_BLOCKS / tiles chunks, then the passes are split evenly over that many
#define GAUSS_SHARED_BLOCKS 1024
#define GAUSS_SHARED_MIN_PASSES 8
static bool gauss_shared_geometry(int64_t N, int64_t D, int K, int* pass_rows, int64_t* passes, int64_t* chunks, int64_t* tiles) {
  if (K < 1 || K > ZK_GAUSS_KMAX_BWD || N <= 0 || D <= 0) return false;
  *tiles = (D + 63) / 64;
  if (*tiles > 65535) return false;  // gridDim.y
  *pass_rows = 4 * (64 / (int)(D < 64 ? D : 64));
  *passes = (N + *pass_rows - 1) / *pass_rows;
  const int64_t cap = GAUSS_SHARED_BLOCKS / *tiles > 1 ? GAUSS_SHARED_BLOCKS / *tiles : 1;
  const int64_t want = (*passes + GAUSS_SHARED_MIN_PASSES - 1) / GAUSS_SHARED_MIN_PASSES;
  *chunks = want < cap ? want : cap;
  return true;
}

__global__ __launch_bounds__(256) void gauss_backward_shared_kernel(GaussSharedArgs a) {
  const int K = a.K, K2 = 2 * K;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t d0 = (int64_t)blockIdx.y * 64;
  const int dw = (int)((a.D - d0) < 64 ? (a.D - d0) : 64);
  const int rpw = 64 / dw;
  float* acc = bw_lds;             // [2K][256]
  float* par = bw_lds + K2 * 256;  // [2K][64]
  const float* src = a.phi + d0 * K2;
  for (int o = tid; o < dw * K2; o += 256) par[(o % K2) * 64 + o / K2] = src[o];
  for (int k = 0; k < K2; ++k) acc[k * 256 + tid] = 0.f;
  __syncthreads();
  const int f = lane % dw, j = lane / dw;
  const int64_t p0 = (int64_t)blockIdx.x * a.passes / gridDim.x, p1 = ((int64_t)blockIdx.x + 1) * a.passes / gridDim.x;
  const int64_t r0 = p0 * a.pass_rows, rr = p1 * a.pass_rows, r1 = rr < a.N ? rr : a.N;
  if (j < rpw) {
    for (int64_t r = r0 + (tid >> 6) * rpw + j; r < r1; r += 4 * rpw) {
      const int64_t e = r * a.D + d0 + f;
      const float glv = a.gl ? (a.gl_reduced ? a.gl[r] : a.gl[e]) : 0.f;
      const float gyv = a.gy ? a.gy[e] : 0.f;
      a.gx[e] = gauss_backward_sweeps(K, [&](int k) { return par[k * 64 + f]; }, [&](int k) { return par[(K + k) * 64 + f]; },
                                      [&](int k, float gb, float ga) { acc[k * 256 + tid] += gb; acc[(K + k) * 256 + tid] += ga; }, a.x[e], gyv, glv);
    }
  }
  __syncthreads();
  // the lanes of one feature in the order (wave, row slot); the sums replace the parameters, which nobody reads any more
  for (int o = tid; o < dw * K2; o += 256) {
    const int k = o / dw, ff = o % dw;
    float s = 0.f;
    for (int w = 0; w < 4; ++w)
      for (int jj = 0; jj < rpw; ++jj) s += acc[k * 256 + w * 64 + jj * dw + ff];
    par[k * 64 + ff] = s;
  }
  __syncthreads();
  float* out = a.work + ((int64_t)blockIdx.x * a.D + d0) * K2;
  for (int o = tid; o < dw * K2; o += 256) out[o] = par[(o % K2) * 64 + o / K2];
}

// gphi[pos] = the chunks' partials of pos: sixteen lanes share a position, lane g adds the chunks [g chunks / 16, (g + 1) chunks / 16) in order, the
// sixteen sums are added in order (one writer per position)
__global__ __launch_bounds__(256) void gauss_shared_reduce_kernel(const float* __restrict__ work, float* __restrict__ gphi, int chunks, int64_t total) {
  __shared__ float part[16][16];
  const int p = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int64_t pos = (int64_t)blockIdx.x * 16 + p;
  float s = 0.f;
  if (pos < total)
    for (int c = (int)((int64_t)g * chunks / 16), c1 = (int)((int64_t)(g + 1) * chunks / 16); c < c1; ++c) s += work[(int64_t)c * total + pos];
  part[g][p] = s;
  __syncthreads();
  if (g == 0 && pos < total) {
    float t = part[0][p];
    for (int i = 1; i < 16; ++i) t += part[i][p];
    gphi[pos] = t;
  }
}

// Any bin count up to 64 (zuko/transforms.py:469-477 accepts any `bins`): one lane per element, knots and softmax probabilities
// in run-time indexed local arrays, parameters read from / gradients written to global memory directly.  A slow path next to the
// K = 4 / 8 / 16 instantiations above, with the same arithmetic (max-subtracted softmax, strict-count bin search, the same
// local vector-Jacobian product).
#define ZK_BWD_MAXK 64
__global__ __launch_bounds__(256) void rqs_backward_generic_kernel(BwdArgs a, int K) {
  const int total = 3 * K - 1;
  const int64_t total_elems = a.N * a.D;
  const float bound = a.bound, ls = a.ls;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total_elems; e += (int64_t)gridDim.x * 256) {
    const float* p = a.phi + e * total;
    float* g = a.gphi + e * total;
    float kn[2][ZK_BWD_MAXK + 1], pr[2][ZK_BWD_MAXK], kd[ZK_BWD_MAXK + 1];
    for (int ax = 0; ax < 2; ++ax) {
      float m = softclip2<float>(p[ax * K], ls);
      for (int j = 1; j < K; ++j) m = fmaxf(m, softclip2<float>(p[ax * K + j], ls));
      float ssum = 0.f;
      for (int j = 0; j < K; ++j) { pr[ax][j] = expf(softclip2<float>(p[ax * K + j], ls) - m); ssum += pr[ax][j]; }
      float cum = 0.f;
      kn[ax][0] = -bound;
      for (int j = 0; j < K; ++j) { pr[ax][j] /= ssum; cum += pr[ax][j]; kn[ax][j + 1] = bound * (2.f * cum - 1.f); }
    }
    kd[0] = kd[K] = 1.f;
    for (int j = 1; j < K; ++j) kd[j] = expf(softclip<float>(p[2 * K + j - 1], ls));
    const float x = a.x[e];
    const float glv = a.gl ? (a.gl_reduced ? a.gl[e / a.D] : a.gl[e]) : 0.f;
    const float gyv = a.gy ? a.gy[e] : 0.f;
    int cnt = 0;
    for (int j = 0; j <= K; ++j) cnt += (kn[0][j] < x) ? 1 : 0;
    const int k = cnt - 1;
    for (int i = 0; i < total; ++i) g[i] = 0.f;
    if (!(k >= 0 && k < K)) { a.gx[e] = gyv; continue; }  // identity outside [-B, B] (and for NaN: no knot compares below it)
    float gv[7];
    rqs_local_vjp(x, kn[0][k], kn[0][k + 1], kn[1][k], kn[1][k + 1], kd[k], kd[k + 1], gyv, glv, gv);
    a.gx[e] = gv[0];
    const float twoB = 2.f * bound;
    float dotw = 0.f, doth = 0.f;
    for (int i = 0; i < K; ++i) {
      dotw += pr[0][i] * twoB * ((i < k ? gv[1] : 0.f) + (i <= k ? gv[2] : 0.f));
      doth += pr[1][i] * twoB * ((i < k ? gv[3] : 0.f) + (i <= k ? gv[4] : 0.f));
    }
    const float cw = fabsf(ls) * 0.5f, cd = fabsf(ls);
    for (int i = 0; i < K; ++i) {
      const float gw = twoB * ((i < k ? gv[1] : 0.f) + (i <= k ? gv[2] : 0.f));
      const float gh = twoB * ((i < k ? gv[3] : 0.f) + (i <= k ? gv[4] : 0.f));
      g[i] = pr[0][i] * (gw - dotw) * softclip_grad(p[i], cw);
      g[K + i] = pr[1][i] * (gh - doth) * softclip_grad(p[K + i], cw);
    }
    if (k >= 1) g[2 * K + k - 1] = gv[5] * kd[k] * softclip_grad(p[2 * K + k - 1], cd);
    if (k + 1 <= K - 1) g[2 * K + k] = gv[6] * kd[k + 1] * softclip_grad(p[2 * K + k], cd);
  }
}

// gz[n, d] = -g[n] (z - loc) / scale^2 ; the ladj gradient is g itself (done by the caller)
__global__ __launch_bounds__(256) void normal_backward_kernel(int64_t N, int64_t D, const float* z, const float* loc, const float* scale, const float* g, float* gz) {
  const int64_t total = N * D;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t d = e % D;
    const float s = scale[d];
    gz[e] = -g[e / D] * (z[e] - loc[d]) / (s * s);
  }
}

// gin = gout * act'(.) expressed through the activation's OUTPUT y (relu, elu, tanh, sigmoid, leaky relu)
__global__ __launch_bounds__(256) void act_backward_kernel(int64_t n, const float* y, const float* gout, int act, float* gin) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const float v = y[e], g = gout[e];
    float d = 1.f;
    switch (act) {
      case 1: d = v > 0.f ? 1.f : 0.f; break;
      case 2: d = v > 0.f ? 1.f : v + 1.f; break;
      case 3: d = 1.f - v * v; break;
      case 6: d = v * (1.f - v); break;
      case 7: d = v > 0.f ? 1.f : 0.01f; break;
      default: break;
    }
    gin[e] = g * d;
  }
}

// seeds of the inverse map's adjoint: gy = gx * exp(-ladj) (= gx / f'(x)), seed = -gy
__global__ __launch_bounds__(256) void inverse_seed_kernel(int64_t n, const float* gx, const float* ladj, float* gy, float* seed) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const float v = gx[e] * expf(-ladj[e]);
    gy[e] = v;
    seed[e] = -v;
  }
}

}  // namespace zk

using namespace zk;

extern "C" {

// kind 0 = affine (phi [N, D, 2] = [shift, scale]), 1 = RQS (phi [N, D, 3K-1]; K in {4, 8, 16} LDS-staged, any other K <= 64 generic); fp32, packed phi/gphi.
int zk_univariate_backward(int kind, int64_t N, int64_t D, int K, double bound, double slope, const void* x, const void* phi, const void* gy, const void* gl,
                           int gl_reduced, void* gx, void* gphi, void* stream) {
  if (N <= 0 || D <= 0) return 0;
  BwdArgs a{};
  a.N = N; a.D = D; a.x = (const float*)x; a.phi = (const float*)phi; a.gy = (const float*)gy; a.gl = (const float*)gl; a.gl_reduced = gl_reduced;
  a.gx = (float*)gx; a.gphi = (float*)gphi; a.bound = (float)bound; a.ls = (float)log(slope);
  if ((((uintptr_t)phi ^ (uintptr_t)gphi) % 16) != 0) return ZK_EINVAL;
  const int total = kind == 0 ? 2 : 3 * K - 1;
  const int64_t tiles = (N * D + 63) / 64;
  const int64_t blocks = (tiles + 3) / 4;
  const size_t lds = 4 * (size_t)(64 * total + 8) * sizeof(float);
  int64_t per_cu = (160 * 1024) / (int64_t)lds;
  per_cu = per_cu > 8 ? 8 : per_cu;
  const int64_t cap = 256 * per_cu;
  const unsigned grid = (unsigned)(blocks < cap ? blocks : cap);
  a.iters = (tiles + (int64_t)grid * 4 - 1) / ((int64_t)grid * 4);
  hipStream_t st = (hipStream_t)stream;
  if (kind == 0) hipLaunchKernelGGL((uni_backward_kernel<0, 1>), dim3(grid), dim3(256), lds, st, a);
  else if (kind == 1 && K == 4) hipLaunchKernelGGL((uni_backward_kernel<1, 4>), dim3(grid), dim3(256), lds, st, a);
  else if (kind == 1 && K == 8) hipLaunchKernelGGL((uni_backward_kernel<1, 8>), dim3(grid), dim3(256), lds, st, a);
  else if (kind == 1 && K == 16) hipLaunchKernelGGL((uni_backward_kernel<1, 16>), dim3(grid), dim3(256), lds, st, a);
  else if (kind == 1 && K >= 1 && K <= ZK_BWD_MAXK) {
    const int64_t nb = (N * D + 255) / 256;
    hipLaunchKernelGGL(rqs_backward_generic_kernel, dim3((unsigned)(nb > 8192 ? 8192 : nb)), dim3(256), 0, st, a, K);
  } else return ZK_EINVAL;
  return ZK_LAUNCH_CHECK();
}

// Gaussianization (phi [N, D, 2K] = [shift(K) | log-scale(K)], 1 <= K <= 32): fp32, packed phi/gphi of the same alignment modulo 16 bytes.
int zk_gauss_backward(int64_t N, int64_t D, int K, const void* x, const void* phi, const void* gy, const void* gl, int gl_reduced, void* gx, void* gphi, void* stream) {
  if (K < 1 || K > ZK_GAUSS_KMAX_BWD) return ZK_EINVAL;
  if ((((uintptr_t)phi ^ (uintptr_t)gphi) % 16) != 0) return ZK_EINVAL;
  if (N <= 0 || D <= 0) return 0;
  BwdArgs a{};
  a.N = N; a.D = D; a.x = (const float*)x; a.phi = (const float*)phi; a.gy = (const float*)gy; a.gl = (const float*)gl; a.gl_reduced = gl_reduced;
  a.gx = (float*)gx; a.gphi = (float*)gphi;
  const int64_t tiles = (N * D + 63) / 64;
  const int64_t blocks = (tiles + 3) / 4;
  const size_t lds = 4 * (size_t)(64 * 2 * K + 8) * sizeof(float);
  if (lds > 64 * 1024) {  // K = 32: 128 bytes of alignment slack above 64 KiB
    const hipError_t e = hipFuncSetAttribute((const void*)gauss_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  int64_t per_cu = (160 * 1024) / (int64_t)lds;
  per_cu = per_cu > 8 ? 8 : per_cu;
  const int64_t cap = 256 * per_cu;
  const unsigned grid = (unsigned)(blocks < cap ? blocks : cap);
  a.iters = (tiles + (int64_t)grid * 4 - 1) / ((int64_t)grid * 4);
  hipLaunchKernelGGL(gauss_backward_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, a, K);
  return ZK_LAUNCH_CHECK();
}

// Floats of `work` for zk_gauss_backward_shared: one [D, 2K] partial per row chunk; <= 0 for a shape the kernel does not serve.
long long int zk_gauss_backward_shared_floats(int64_t N, int64_t D, int K) {
  int pass_rows;
  int64_t passes, chunks, tiles;
  if (!gauss_shared_geometry(N, D, K, &pass_rows, &passes, &chunks, &tiles)) return 0;
  return chunks * D * 2 * K;
}

// Gaussianization with parameters shared by all rows (phi [D, 2K] = [shift(K) | log-scale(K)], 1 <= K <= 32): gx [N, D] and gphi [D, 2K] summed over the rows.
int zk_gauss_backward_shared(int64_t N, int64_t D, int K, const void* x, const void* phi, const void* gy, const void* gl, int gl_reduced, void* gx, void* work,
                             void* gphi, void* stream) {
  if (K < 1 || K > ZK_GAUSS_KMAX_BWD) return ZK_EINVAL;
  if ((((uintptr_t)phi | (uintptr_t)gphi) % 16) != 0) return ZK_EINVAL;
  if (N <= 0 || D <= 0) return 0;
  GaussSharedArgs a{};
  int64_t chunks, tiles;
  if (!gauss_shared_geometry(N, D, K, &a.pass_rows, &a.passes, &chunks, &tiles)) return ZK_EINVAL;
  if (!x || !phi || !gx || !work || !gphi) return ZK_EINVAL;
  a.N = N; a.D = D; a.K = K; a.x = (const float*)x; a.phi = (const float*)phi; a.gy = (const float*)gy; a.gl = (const float*)gl; a.gl_reduced = gl_reduced;
  a.gx = (float*)gx; a.work = (float*)work;
  const size_t lds = (size_t)(256 + 64) * 2 * K * sizeof(float);
  if (lds > 64 * 1024) {  // K >= 26; 80 KiB at K = 32
    const hipError_t e = hipFuncSetAttribute((const void*)gauss_backward_shared_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gauss_backward_shared_kernel, dim3((unsigned)chunks, (unsigned)tiles), dim3(256), lds, st, a);
  const int rc = ZK_LAUNCH_CHECK();
  if (rc != 0) return rc;
  const int64_t total = D * 2 * K;
  hipLaunchKernelGGL(gauss_shared_reduce_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, st, (const float*)work, (float*)gphi, (int)chunks, total);
  return ZK_LAUNCH_CHECK();
}

int zk_diag_normal_backward(int64_t N, int64_t D, const void* z, const void* loc, const void* scale, const void* g, void* gz, void* stream) {
  if (N <= 0 || D <= 0) return 0;
  const int64_t nb = (N * D + 255) / 256;
  hipLaunchKernelGGL(normal_backward_kernel, dim3((unsigned)(nb > 4096 ? 4096 : nb)), dim3(256), 0, (hipStream_t)stream, N, D, (const float*)z, (const float*)loc,
                     (const float*)scale, (const float*)g, (float*)gz);
  return ZK_LAUNCH_CHECK();
}

int zk_inverse_seed(int64_t n, const void* gx, const void* ladj, void* gy, void* seed, void* stream) {
  if (n <= 0) return 0;
  const int64_t nb = (n + 255) / 256;
  hipLaunchKernelGGL(inverse_seed_kernel, dim3((unsigned)(nb > 4096 ? 4096 : nb)), dim3(256), 0, (hipStream_t)stream, n, (const float*)gx, (const float*)ladj, (float*)gy, (float*)seed);
  return ZK_LAUNCH_CHECK();
}

int zk_act_backward(int64_t n, const void* y, const void* gout, int act, void* gin, void* stream) {
  if (n <= 0) return 0;
  if (!(act == 0 || act == 1 || act == 2 || act == 3 || act == 6 || act == 7)) return ZK_EINVAL;
  const int64_t nb = (n + 255) / 256;
  hipLaunchKernelGGL(act_backward_kernel, dim3((unsigned)(nb > 4096 ? 4096 : nb)), dim3(256), 0, (hipStream_t)stream, n, (const float*)y, (const float*)gout, act, (float*)gin);
  return ZK_LAUNCH_CHECK();
}

}  // extern "C"
