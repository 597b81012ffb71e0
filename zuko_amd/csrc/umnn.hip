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
// Execution model (gfx950) — the one of csrc/mnn.hip; the image layout, the signal product, the launch geometry and the launch are the same code
// (csrc/zk_mnn_common.h), the network behind the first layer and the __global__ body are this file's own:
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
#include "zk_mnn_common.h"

namespace zk {

#define UMNN_QUAD_MAX 64  // nodes of the quadrature table: 512 bytes of LDS behind the image

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
  MnnLayout L;
};

// x / (1 + |x / 7|): the integrand's logarithm, within (-7, 7) (zuko/flows/neural.py:104)
__device__ __forceinline__ float umnn_squash(float h) { return h / (1.f + fabsf(h / 7.f)); }

// one hidden-to-hidden layer for NP evaluation points at once: v[p] <- ELU(W v[p] + b); tin / tout tiles.  One read of a weight fragment feeds
// the accumulators of all points.
template <int TM, int NP>
__device__ __forceinline__ void umnn_hidden(const float* W, const float* B, int tin, int tout, int lane, int q, mnn_f4 (&v)[NP * TM]) {
  mnn_f4 ov[NP * TM];
  const int rowstride = tin * 256;  // the tiles of one out tile are consecutive: the in tile is an immediate offset of the read
  mnn_for<TM>([&](auto o) MNN_INLINE {
    if (o < tout) {
      const float* const p0 = W + o * rowstride + lane * 4;
      const mnn_f4 b = *reinterpret_cast<const mnn_f4*>(B + o * 16 + q * 4);
      mnn_for<NP>([&](auto p) MNN_INLINE { ov[p * TM + o] = b; });
      mnn_for<TM>([&](auto it) MNN_INLINE {
        if (it < tin) {
          const mnn_f4 a0 = *reinterpret_cast<const mnn_f4*>(p0 + it * 256);
          mnn_for<4>([&](auto r) MNN_INLINE {
            mnn_for<NP>([&](auto p) MNN_INLINE {
              ov[p * TM + o] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[(int)r], v[p * TM + it][(int)r], ov[p * TM + o], 0, 0, 0);
            });
          });
        }
      });
    }
  });
  mnn_for<TM>([&](auto o) MNN_INLINE {
    if (o < tout) {
      mnn_for<NP>([&](auto p) MNN_INLINE {
        mnn_for<4>([&](auto r) MNN_INLINE { v[p * TM + o][(int)r] = mnn_elu(ov[p * TM + o][(int)r]); });
      });
    }
  });
}

// the integrand network behind the first layer's pre-activation at NP points u[p] of the element this lane belongs to: h[p] = h(u[p], signal)
template <int TM, int NP>
__device__ __forceinline__ void umnn_tail(const MnnLayout& L, const float* lds, int lane, int q, const float (&u)[NP], const mnn_f4 (&c0)[TM], float (&h)[NP]) {
  mnn_f4 v[NP * TM];
  mnn_for<TM>([&](auto o) MNN_INLINE {
    if (o < L.T[0]) {
      const mnn_f4 w = *reinterpret_cast<const mnn_f4*>(lds + L.o_w0x + o * 16 + q * 4);
      mnn_for<NP>([&](auto p) MNN_INLINE {
        mnn_for<4>([&](auto r) MNN_INLINE { v[p * TM + o][(int)r] = mnn_elu(fmaf(w[(int)r], u[p], c0[o][(int)r])); });
      });
    }
  });
  if (L.nh > 1) umnn_hidden<TM, NP>(lds + L.o_w[1], lds + L.o_b[1], L.T[0], L.T[1], lane, q, v);
  if (L.nh > 2) umnn_hidden<TM, NP>(lds + L.o_w[2], lds + L.o_b[2], L.T[1], L.T[2], lane, q, v);
  const int tl = L.T[L.nh - 1];
  float py[NP];
  mnn_for<NP>([&](auto p) MNN_INLINE { py[p] = 0.f; });
  mnn_for<TM>([&](auto o) MNN_INLINE {
    if (o < tl) {
      const mnn_f4 w = *reinterpret_cast<const mnn_f4*>(lds + L.o_wl + o * 16 + q * 4);
      mnn_for<NP>([&](auto p) MNN_INLINE {
        mnn_for<4>([&](auto r) MNN_INLINE { py[p] = fmaf(w[(int)r], v[p * TM + o][(int)r], py[p]); });
      });
    }
  });
  const float bl = lds[L.o_bl];
  mnn_for<NP>([&](auto p) MNN_INLINE { h[p] = mnn_sum_q(py[p]) + bl; });
}

// f(x) = x sum_i w_i g(t_i x), i = 0, 1, ... in that order; with LADJ also hx = h(x), as one more point behind the nodes.  The points go through
// the network two at a time; a last odd one alone.
template <int TM, bool LADJ>
__device__ __forceinline__ float umnn_integral(const MnnLayout& L, const float* lds, const float* qt, int nq, int lane, int q, float x, const mnn_f4 (&c0)[TM], float& hx) {
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

template <int TM, bool INVERSE> __global__ __launch_bounds__(MNN_THREADS, 2) void umnn_kernel(UmnnArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
  const MnnLayout& L = a.L;
  const int nq = a.n_quad;
  float* const qt = umnn_lds + L.total;  // nodes [nq], weights [nq] (not touched by the image loads below)
  for (int i = tid; i < 2 * nq; i += MNN_THREADS) qt[i] = a.quad[i];
  const long long row0 = (long long)blockIdx.x * a.rows_per_block;
  for (int fc = 0; fc < a.feats_per_block; ++fc) {
    const int col = blockIdx.y * a.feats_per_block + fc;
    if (col >= a.Dsel) break;  // (uniform over the block)
    int f = a.feat ? a.feat[col] : col;
    f = f < 0 ? 0 : (f >= a.n_features ? a.n_features - 1 : f);  // (a memory guard only: the caller checks the range, zuko_amd/ops.py: _mnn_feat)
    const float* img = a.image + (size_t)f * L.total;
    __syncthreads();  // the previous column's image is no longer read
    mnn_stage_image(umnn_lds, img, L.total, tid);
    __syncthreads();
    for (int tile = wave; tile * 16 < a.rows_per_block && row0 + tile * 16 < a.N; tile += MNN_THREADS / 64) {
      const long long row = row0 + tile * 16 + j;
      const long long rc = row < a.N ? row : a.N - 1;  // rows behind the end compute on the last row and store nothing
      const float xin = a.x[rc * a.ldx + col];
      const float cst = a.constant ? a.constant[rc * a.ldc + col * a.ldccol] : 0.f;
      mnn_f4 c0[TM];
      mnn_signal<TM>(L, umnn_lds, a.signal + rc * a.lds + col * a.ldcol, lane, q, c0);
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

template <bool INVERSE> static int umnn_launch(const zk_umnn_args_v1* p, void* stream) {
  UmnnArgs a;
  dim3 grid;
  const int err = mnn_prepare<INVERSE>(p, &a, &grid, [](const zk_umnn_args_v1& b) {
    return b.n_quad >= 1 && b.n_quad <= UMNN_QUAD_MAX && b.ld_col >= b.S && b.ld_signal >= (b.Dsel - 1) * b.ld_col + b.S && b.ld_constant >= 0 && b.ld_constant_col >= 0;
  });
  if (err != 0 || grid.x == 0) return err;
  if (!p->quad) return ZK_EINVAL;
  a.constant = (const float*)p->constant; a.quad = (const float*)p->quad;
  a.ldcol = p->ld_col; a.ldc = p->ld_constant; a.ldccol = p->ld_constant_col; a.n_quad = p->n_quad;
  hipStream_t st = (hipStream_t)stream;
  const bool small = a.L.T[0] <= 4 && a.L.T[1] <= 4 && a.L.T[2] <= 4;
  const void* fn = small ? (const void*)umnn_kernel<4, INVERSE> : (const void*)umnn_kernel<8, INVERSE>;
  const int rc = mnn_launch_dyn_lds(fn, grid, (a.L.total + 2 * UMNN_QUAD_MAX) * 4, &a, st);
  if (rc != 0 || INVERSE || !p->ladj_reduced) return rc;
  return mnn_rowsum((const float*)p->work, (float*)p->ladj, a.N, a.Dsel, st);
}

}  // namespace zk

extern "C" int zk_umnn_forward(const zk_umnn_args_v1* args, void* stream) { return zk::umnn_launch<false>(args, stream); }
extern "C" int zk_umnn_inverse(const zk_umnn_args_v1* args, void* stream) { return zk::umnn_launch<true>(args, stream); }
extern "C" int zk_umnn_launch_geometry(int64_t N, int64_t Dsel, int* rows_per_block, int* feats_per_block) { return zk::mnn_geometry(N, Dsel, rows_per_block, feats_per_block); }
