// zuko_amd — unconstrained monotone neural network of the unconstrained neural autoregressive flow (UNAF): Gauss-Legendre quadrature of a
// positive integrand network, its log-derivative and the bisection inverse.
//
// Replaces UMNN.g + UnconstrainedMonotonicTransform.call_and_ladj + AdditiveTransform (zuko/flows/neural.py:100-118, zuko/transforms.py:911-924,
// zuko/utils.py:328-363):
//     sq(v) = v / (1 + |v / 7|),  g(u) = exp(sq(h(u, signal))),  f(x) = x sum_i w_i g(t_i x),  y = f(x) + constant,  ladj = sq(h(x, signal))
// (the reference: stacked einsums over a [n_quad, N, D, 1 + S] tensor) and MonotonicTransform._inverse + Bisection.forward (zuko/transforms.py:
// 609-617, zuko/utils.py:170-178).  Every feature f owns an integrand network h: (1 + S) -> H1 [-> H2 [-> H3]] -> 1 with signed weights and
// ELU(alpha = 1); an element (n, d) evaluates it n_quad + 1 times in the forward direction and n_bisect * n_quad times in the inverse one.
//
// Execution model (gfx950) — the one of csrc/mnn.hip, whose routines are restated here so that zk_mnn_* keep their code:
//   * a wavefront owns 16 elements of ONE feature; every layer runs transposed on v_mfma_f32_16x16x4_f32 (exact fp32) with the weight image of
//     zuko_amd/mnn_plan.py (here of the signed weights) in LDS, the activations stay in registers in the D layout (lane (j, q) = (lane & 15,
//     lane >> 4) holds out units 16 t + 4 q + r of element j);
//   * the signal's share of the first layer, W0[:, 1:] signal + b0, is computed ONCE per element; every evaluation of h starts from it with one
//     multiply-add per unit;
//   * the evaluations of an element are independent: TWO of them run through the layers together — every weight fragment read from LDS feeds two
//     accumulator chains, and the ELU's expm1 of one point overlaps the matrix instructions of the other.  No tangent is carried: ladj is
//     sq(h(x)), the value of one more evaluation;
//   * the quadrature table (nodes, then weights; float32 of numpy's float64 rule, made on the host) sits in LDS behind the image; the sum over the
//     nodes runs in the order i = 0, 1, ... whatever the pairing;
//   * no atomics: ladj[N] is a second launch that adds the columns of a row in order.
//
// An element's y / ladj depends on its own x, signal, constant and feature only: not on N, Dsel, the strides, the launch geometry or its neighbours.
#include "../../include/zuko_amd.h"
#include "zk_common.h"
#include <mutex>
#include <unordered_map>
#include <utility>

namespace zk {

typedef float umnn_f4 __attribute__((ext_vector_type(4)));

#define UMNN_INLINE __attribute__((always_inline))
#define UMNN_LDS_MAX (128 * 1024)  // bound on one feature's image (MNN_LDS_MAX of csrc/mnn.hip); the quadrature table adds at most 512 bytes
#define UMNN_THREADS 256
#define UMNN_QUAD_MAX 64

template <class F, int... I> __device__ __forceinline__ void umnn_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F> __device__ __forceinline__ void umnn_for(F&& f) { umnn_for_impl(f, std::make_integer_sequence<int, N>{}); }

// Offsets (floats) of one feature's image: the arithmetic of zuko_amd/mnn_plan.py: layout and of csrc/mnn.hip: mnn_layout (the launch compares
// its total with zk_mnn_image_floats, the size oracle).
struct UmnnLayout {
  int nh, S, ks;  // hidden layers, signal features, k-steps of the signal product = ceil(S / 4)
  int T[3];       // 16-unit tiles per hidden layer
  int o_w0s, o_w0x, o_b0, o_w[3], o_b[3], o_wl, o_bl, total;
};

static inline bool umnn_layout(int S, int nh, const int* widths, UmnnLayout* L) {
  if (S < 1 || S > 63 || nh < 1 || nh > 3) return false;
  for (int l = 0; l < 3; ++l) {
    const int h = l < nh ? widths[l] : 0;
    if (l < nh ? (h < 16 || h > 128 || h % 16 != 0) : h != 0) return false;
    L->T[l] = h / 16;
  }
  L->nh = nh; L->S = S; L->ks = (S + 3) / 4;
  int o = 0;
  L->o_w0s = o; o += L->T[0] * L->ks * 64;
  L->o_w0x = o; o += L->T[0] * 16;
  L->o_b0 = o; o += L->T[0] * 16;
  L->o_w[0] = L->o_b[0] = 0;
  for (int l = 1; l < 3; ++l) {
    L->o_w[l] = o; if (l < nh) o += L->T[l] * L->T[l - 1] * 256;
    L->o_b[l] = o; if (l < nh) o += L->T[l] * 16;
  }
  L->o_wl = o; o += L->T[nh - 1] * 16;
  L->o_bl = o; o += 4;
  L->total = o;
  return o * 4 <= UMNN_LDS_MAX;
}

struct UmnnArgs {
  const float* x;         // forward: x; inverse: y
  const float* signal;
  const float* constant;  // or nullptr
  const float* image;
  const float* quad;
  const int* feat;
  float* y;               // forward: y; inverse: the solutions
  float* ladj;            // [N, Dsel] (the per-element buffer, also when the caller asked for the row sums)
  long long N, ldx, lds, ldcol, ldy, ldc, ldccol;
  int Dsel, n_features, rows_per_block, feats_per_block, n_bisect, n_quad;
  float bound;
  UmnnLayout L;
};

__device__ __forceinline__ float umnn_elu(float p) { return p > 0.f ? p : expm1f(p); }
// x / (1 + |x / 7|): the integrand's logarithm, within (-7, 7) (zuko/flows/neural.py:104)
__device__ __forceinline__ float umnn_squash(float h) { return h / (1.f + fabsf(h / 7.f)); }

// c0 = W0[:, 1:] signal + b0 in the D layout (T1 tiles)
template <int TM> __device__ __forceinline__ void umnn_signal(const UmnnLayout& L, const float* lds, const float* __restrict__ sp, int lane, int q, umnn_f4 (&c0)[TM]) {
  float sig[16];
  umnn_for<16>([&](auto s) UMNN_INLINE {
    sig[s] = 0.f;
    if (s < L.ks) sig[s] = (4 * s + q < L.S) ? sp[4 * s + q] : 0.f;
  });
  umnn_for<TM>([&](auto o) UMNN_INLINE {
    if (o < L.T[0]) c0[o] = *reinterpret_cast<const umnn_f4*>(lds + L.o_b0 + o * 16 + q * 4);
  });
  const float* const pw = lds + L.o_w0s + lane;  // (tile o, k-step s at o * ostride + 64 s: the k-step is an immediate offset of the read)
  const int ostride = L.ks * 64;
  umnn_for<16>([&](auto s) UMNN_INLINE {
    if (s < L.ks) {
      umnn_for<TM>([&](auto o) UMNN_INLINE {
        if (o < L.T[0]) c0[o] = __builtin_amdgcn_mfma_f32_16x16x4f32(pw[o * ostride + s * 64], sig[s], c0[o], 0, 0, 0);
      });
    }
  });
}

// one hidden-to-hidden layer for NP evaluation points at once: v[p] <- ELU(W v[p] + b); tin / tout tiles.  One read of a weight fragment feeds
// the accumulators of all points.
template <int TM, int NP>
__device__ __forceinline__ void umnn_hidden(const float* W, const float* B, int tin, int tout, int lane, int q, umnn_f4 (&v)[NP * TM]) {
  umnn_f4 ov[NP * TM];
  const int rowstride = tin * 256;  // the tiles of one out tile are consecutive: the in tile is an immediate offset of the read
  umnn_for<TM>([&](auto o) UMNN_INLINE {
    if (o < tout) {
      const float* const p0 = W + o * rowstride + lane * 4;
      const umnn_f4 b = *reinterpret_cast<const umnn_f4*>(B + o * 16 + q * 4);
      umnn_for<NP>([&](auto p) UMNN_INLINE { ov[p * TM + o] = b; });
      umnn_for<TM>([&](auto it) UMNN_INLINE {
        if (it < tin) {
          const umnn_f4 a0 = *reinterpret_cast<const umnn_f4*>(p0 + it * 256);
          umnn_for<4>([&](auto r) UMNN_INLINE {
            umnn_for<NP>([&](auto p) UMNN_INLINE {
              ov[p * TM + o] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[(int)r], v[p * TM + it][(int)r], ov[p * TM + o], 0, 0, 0);
            });
          });
        }
      });
    }
  });
  umnn_for<TM>([&](auto o) UMNN_INLINE {
    if (o < tout) {
      umnn_for<NP>([&](auto p) UMNN_INLINE {
        umnn_for<4>([&](auto r) UMNN_INLINE { v[p * TM + o][(int)r] = umnn_elu(ov[p * TM + o][(int)r]); });
      });
    }
  });
}

// sum over the four lanes (j, 0..3) that hold one element: the same value in all four, the same order everywhere
__device__ __forceinline__ float umnn_sum_q(float p) {
  p += __shfl_xor(p, 16, 64);
  p += __shfl_xor(p, 32, 64);
  return p;
}

// the integrand network behind the first layer's pre-activation at NP points u[p] of the element this lane belongs to: h[p] = h(u[p], signal)
template <int TM, int NP>
__device__ __forceinline__ void umnn_tail(const UmnnLayout& L, const float* lds, int lane, int q, const float (&u)[NP], const umnn_f4 (&c0)[TM], float (&h)[NP]) {
  umnn_f4 v[NP * TM];
  umnn_for<TM>([&](auto o) UMNN_INLINE {
    if (o < L.T[0]) {
      const umnn_f4 w = *reinterpret_cast<const umnn_f4*>(lds + L.o_w0x + o * 16 + q * 4);
      umnn_for<NP>([&](auto p) UMNN_INLINE {
        umnn_for<4>([&](auto r) UMNN_INLINE { v[p * TM + o][(int)r] = umnn_elu(fmaf(w[(int)r], u[p], c0[o][(int)r])); });
      });
    }
  });
  if (L.nh > 1) umnn_hidden<TM, NP>(lds + L.o_w[1], lds + L.o_b[1], L.T[0], L.T[1], lane, q, v);
  if (L.nh > 2) umnn_hidden<TM, NP>(lds + L.o_w[2], lds + L.o_b[2], L.T[1], L.T[2], lane, q, v);
  const int tl = L.T[L.nh - 1];
  float py[NP];
  umnn_for<NP>([&](auto p) UMNN_INLINE { py[p] = 0.f; });
  umnn_for<TM>([&](auto o) UMNN_INLINE {
    if (o < tl) {
      const umnn_f4 w = *reinterpret_cast<const umnn_f4*>(lds + L.o_wl + o * 16 + q * 4);
      umnn_for<NP>([&](auto p) UMNN_INLINE {
        umnn_for<4>([&](auto r) UMNN_INLINE { py[p] = fmaf(w[(int)r], v[p * TM + o][(int)r], py[p]); });
      });
    }
  });
  const float bl = lds[L.o_bl];
  umnn_for<NP>([&](auto p) UMNN_INLINE { h[p] = umnn_sum_q(py[p]) + bl; });
}

// f(x) = x sum_i w_i g(t_i x), i = 0, 1, ... in that order; with LADJ also hx = h(x), as one more point behind the nodes.  The points go through
// the network two at a time; a last odd one alone.
template <int TM, bool LADJ>
__device__ __forceinline__ float umnn_integral(const UmnnLayout& L, const float* lds, const float* qt, int nq, int lane, int q, float x, const umnn_f4 (&c0)[TM], float& hx) {
  const int m = nq + (LADJ ? 1 : 0);
  float acc = 0.f;
  int k = 0;
  for (; k + 1 < m; k += 2) {
    const bool node1 = !LADJ || k + 1 < nq;  // (uniform) the second point is a node, not x itself
    const float u[2] = {qt[k] * x, node1 ? qt[k + 1] * x : x};
    float h[2];
    umnn_tail<TM, 2>(L, lds, lane, q, u, c0, h);
    acc = acc + qt[nq + k] * expf(umnn_squash(h[0]));
    if (node1) acc = acc + qt[nq + k + 1] * expf(umnn_squash(h[1]));
    else hx = h[1];
  }
  if (k < m) {
    const bool node = !LADJ || k < nq;
    const float u[1] = {node ? qt[k] * x : x};
    float h[1];
    umnn_tail<TM, 1>(L, lds, lane, q, u, c0, h);
    if (node) acc = acc + qt[nq + k] * expf(umnn_squash(h[0]));
    else hx = h[0];
  }
  return x * acc;
}

extern __shared__ __attribute__((aligned(16))) float umnn_lds[];

template <int TM, bool INVERSE> __global__ __launch_bounds__(UMNN_THREADS, 2) void umnn_kernel(UmnnArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
  const UmnnLayout& L = a.L;
  const int nq = a.n_quad;
  float* const qt = umnn_lds + L.total;  // nodes [nq], weights [nq] (not touched by the image loads below)
  for (int i = tid; i < 2 * nq; i += UMNN_THREADS) qt[i] = a.quad[i];
  const long long row0 = (long long)blockIdx.x * a.rows_per_block;
  for (int fc = 0; fc < a.feats_per_block; ++fc) {
    const int col = blockIdx.y * a.feats_per_block + fc;
    if (col >= a.Dsel) break;  // (uniform over the block)
    int f = a.feat ? a.feat[col] : col;
    f = f < 0 ? 0 : (f >= a.n_features ? a.n_features - 1 : f);  // (a memory guard only: the caller checks the range, zuko_amd/ops.py: _mnn_feat)
    const float* img = a.image + (size_t)f * L.total;
    __syncthreads();  // the previous column's image is no longer read
    for (int i = tid * 4; i < L.total; i += UMNN_THREADS * 4) *reinterpret_cast<umnn_f4*>(umnn_lds + i) = *reinterpret_cast<const umnn_f4*>(img + i);
    __syncthreads();
    for (int tile = wave; tile * 16 < a.rows_per_block && row0 + tile * 16 < a.N; tile += UMNN_THREADS / 64) {
      const long long row = row0 + tile * 16 + j;
      const long long rc = row < a.N ? row : a.N - 1;  // rows behind the end compute on the last row and store nothing
      const float xin = a.x[rc * a.ldx + col];
      const float cst = a.constant ? a.constant[rc * a.ldc + col * a.ldccol] : 0.f;
      umnn_f4 c0[TM];
      umnn_signal<TM>(L, umnn_lds, a.signal + rc * a.lds + col * a.ldcol, lane, q, c0);
      if constexpr (!INVERSE) {
        float hx = 0.f;
        const float fx = umnn_integral<TM, true>(L, umnn_lds, qt, nq, lane, q, xin, c0, hx);
        if (q == 0 && row < a.N) {
          a.y[row * a.ldy + col] = fx + cst;
          a.ladj[row * a.Dsel + col] = umnn_squash(hx);
        }
      } else {
        // zuko/utils.py:170-178 in fp32: n times c = (a + b) / 2, f(c) < y ? a = c : b = c; the answer is the last midpoint
        const float target = xin - cst;  // (AdditiveTransform's inverse comes first: zuko/transforms.py:141-150)
        float lo = -a.bound, hi = a.bound;
        for (int it = 0; it < a.n_bisect; ++it) {
          const float c = (lo + hi) / 2;
          float unused;
          const float fy = umnn_integral<TM, false>(L, umnn_lds, qt, nq, lane, q, c, c0, unused);
          const bool below = fy < target;
          lo = below ? c : lo;
          hi = below ? hi : c;
        }
        if (q == 0 && row < a.N) a.y[row * a.ldy + col] = (lo + hi) / 2;
      }
    }
  }
}

// ladj[n] = the columns of row n added left to right
__global__ __launch_bounds__(256) void umnn_rowsum_kernel(const float* __restrict__ e, float* __restrict__ out, long long N, int D) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int d = 0; d < D; ++d) s += e[n * D + d];
  out[n] = s;
}

// Grant, launch, check (as mnn_launch_dyn_lds of csrc/mnn.hip): the opt-in to more than 64 KiB of dynamic LDS is per function, set under a lock,
// once, and again only if a larger size is asked for.
static int umnn_launch_dyn_lds(const void* fn, dim3 grid, int lds_bytes, UmnnArgs& a, hipStream_t st) {
  hipError_t e = hipSuccess;
  {
    static std::mutex mu;
    static std::unordered_map<const void*, int> granted;
    std::lock_guard<std::mutex> lock(mu);
    int& g = granted[fn];
    if (g < lds_bytes) {
      e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
      if (e != hipSuccess) return (int)e;
      g = lds_bytes;
    }
  }
  void* kargs[] = {&a};
  e = hipLaunchKernel(fn, grid, dim3(UMNN_THREADS), kargs, lds_bytes, st);
  if (e != hipSuccess) return (int)e;
  return ZK_LAUNCH_CHECK();
}

template <bool INVERSE> static int umnn_launch(const zk_umnn_args_v1* p, void* stream) {
  if (!p || p->struct_size != sizeof(zk_umnn_args_v1) || p->version != 1) return ZK_EINVAL;  // (argument block: include/zuko_amd.h)
  UmnnArgs a;
  const int widths[3] = {p->width0, p->width1, p->width2};
  if (!umnn_layout(p->S, p->n_hidden, widths, &a.L)) return ZK_EINVAL;
  if (a.L.total != zk_mnn_image_floats(p->S, p->n_hidden, p->width0, p->width1, p->width2)) return ZK_EINVAL;  // (the two layouts are one)
  if (p->image_floats != a.L.total || p->n_features < 1 || p->N < 0 || p->Dsel < 1 || p->Dsel > (1 << 20)) return ZK_EINVAL;
  if (p->n_quad < 1 || p->n_quad > UMNN_QUAD_MAX) return ZK_EINVAL;
  if (p->ldx < 1 || p->ldy < p->Dsel || p->ld_col < p->S || p->ld_signal < (p->Dsel - 1) * p->ld_col + p->S) return ZK_EINVAL;
  if (p->ld_constant < 0 || p->ld_constant_col < 0) return ZK_EINVAL;
  if (INVERSE && (p->n_bisect < 0 || p->n_bisect > 64 || !(p->bound > 0))) return ZK_EINVAL;
  if (p->N == 0) return 0;
  if (!p->x || !p->signal || !p->image || !p->quad || !p->y) return ZK_EINVAL;
  if (!INVERSE && (!p->ladj || (p->ladj_reduced && !p->work))) return ZK_EINVAL;
  a.x = (const float*)p->x; a.signal = (const float*)p->signal; a.constant = (const float*)p->constant; a.image = (const float*)p->image;
  a.quad = (const float*)p->quad; a.feat = (const int*)p->feat;
  a.y = (float*)p->y; a.ladj = (float*)(p->ladj_reduced ? p->work : p->ladj);
  a.N = p->N; a.ldx = p->ldx; a.lds = p->ld_signal; a.ldcol = p->ld_col; a.ldy = p->ldy; a.ldc = p->ld_constant; a.ldccol = p->ld_constant_col;
  a.Dsel = (int)p->Dsel; a.n_features = p->n_features; a.n_bisect = p->n_bisect; a.n_quad = p->n_quad; a.bound = (float)p->bound;
  if (zk_umnn_launch_geometry(a.N, a.Dsel, &a.rows_per_block, &a.feats_per_block) != 0) return ZK_EINVAL;  // (results do not depend on it)
  const long long cols = (a.Dsel + a.feats_per_block - 1) / a.feats_per_block;
  const long long gx = (a.N + a.rows_per_block - 1) / a.rows_per_block;
  if (gx > 0x7fffffffLL || cols > 65535) return ZK_EINVAL;
  const dim3 grid((unsigned)gx, (unsigned)cols);
  const int lds_bytes = (a.L.total + 2 * UMNN_QUAD_MAX) * 4;
  hipStream_t st = (hipStream_t)stream;
  const bool small = a.L.T[0] <= 4 && a.L.T[1] <= 4 && a.L.T[2] <= 4;
  const void* fn = small ? (const void*)umnn_kernel<4, INVERSE> : (const void*)umnn_kernel<8, INVERSE>;
  int err = umnn_launch_dyn_lds(fn, grid, lds_bytes, a, st);
  if (err != 0 || INVERSE || !p->ladj_reduced) return err;
  hipLaunchKernelGGL(umnn_rowsum_kernel, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, st, (const float*)p->work, (float*)p->ladj, a.N, a.Dsel);
  return ZK_LAUNCH_CHECK();
}

}  // namespace zk

extern "C" int zk_umnn_forward(const zk_umnn_args_v1* args, void* stream) { return zk::umnn_launch<false>(args, stream); }
extern "C" int zk_umnn_inverse(const zk_umnn_args_v1* args, void* stream) { return zk::umnn_launch<true>(args, stream); }
// The launch geometry of an [N, Dsel] call (the rule of zk_mnn_launch_geometry, restated as the kernels are): enough blocks for 256 CUs first,
// then longer runs per image load.  A pure function of the two sizes.
extern "C" int zk_umnn_launch_geometry(int64_t N, int64_t Dsel, int* rows_per_block, int* feats_per_block) {
  if (N < 1 || Dsel < 1 || Dsel > (1 << 20) || !rows_per_block || !feats_per_block) return ZK_EINVAL;
  const long long t64 = (N + 63) / 64;
  const int feats = t64 * ((Dsel + 3) / 4) >= 512 ? 4 : 1;
  const long long cols = (Dsel + feats - 1) / feats;
  int rows = 256;
  while (rows > 64 && ((N + rows - 1) / rows) * cols < 1024) rows /= 2;
  *rows_per_block = rows;
  *feats_per_block = feats;
  return 0;
}
