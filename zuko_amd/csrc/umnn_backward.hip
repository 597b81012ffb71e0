// zuko_amd — adjoint of the unconstrained monotone neural network of the unconstrained neural autoregressive flow (UNAF): the gradients of
// (y, ladj) of csrc/umnn.hip with respect to x, the signal and every weight and bias of the per-feature integrand networks.
//
// Per element (n, column j of feature f), with q0 = W0[:, 1:] s + b0 formed once, the points u_i = t_i x (i < n_quad) and u = x:
//     forward of a point    p_0 = W0[:, 0] u + q0     a_l = elu(p_l)     p_l = W_l a_{l-1} + b_l     h = w_last . a_last + b_last
//                           sq = h / (1 + |h| / 7)    g = exp(sq)        y = x sum_i w_i g_i + constant      ladj = sq(h(x))
//     upstream on h         node i: hb = gy x w_i g_i sq'(h_i)      the point x: hb = gl sq'(h_x)      sq'(h) = 1 / (1 + |h| / 7)^2
//     reverse sweep         g w_last += hb a_last    g b_last += hb    ab = hb w_last
//                           pb_l = ab_l elu'(p_l)    g W_l += pb_l a_{l-1}^T    g b_l += pb_l    ab_{l-1} = W_l^T pb_l
//     first layer           g W0[:, 0] += pb_0 u     P0 = sum over the points of pb_0;  after the last point:
//                           g b0 += P0    g W0[:, 1:] += P0 s^T    gsignal = W0[:, 1:]^T P0          (once per element, not once per point)
//     gx = gy g(x) + W0[:, 0] . pb_0(x): the integrand at the upper limit (zuko/utils.py:282-326), not the derivative of the quadrature sum; the
//     nodes t_i x carry no gradient to x.  The constant's gradient is gy itself: the caller's.
// No tangent chains and no second derivative of the activation: ladj is the value of one more evaluation.  The sums over the points run in the
// order i = 0, 1, ..., then x.
//
// Execution model (gfx950): that of csrc/mnn_backward.hip, whose layouts, geometry, transposes, partial stores and chunk reduction it shares
// (csrc/zk_mnn_bwd_common.h) —
//   * a wavefront owns 16 elements of ONE feature; the backward image of the SIGNED weights (zuko_amd/mnn_plan.py: layout_backward) sits in LDS, the
//     quadrature table (nodes, then weights) behind the transpose scratch; the forward is recomputed from x and the signal, two points at a time (a
//     last odd one alone; one at a time with three hidden layers), with their pre-activations and activations in registers; nothing else is read;
//   * the weight gradients contract over the wave's 16 elements through the per-wave LDS transpose (s_waitcnt + wave barrier, no workgroup barrier
//     inside the row loop) and stay in accumulator registers across the points and the row tiles a wave walks;
//   * a block adds its four waves in LDS in the order 0, 1, 2, 3 and writes ONE partial per (row chunk, column); mnn_bwd_reduce adds the partials in
//     chunk order and scatters them into the flat parameter order WITHOUT sign(W): these weights are signed.  No atomics: the same inputs give the
//     same bits.
#include "zk_mnn_bwd_common.h"

namespace zk {

#define UMNN_QUAD_MAX 64  // nodes of the quadrature table (csrc/umnn.hip): 512 bytes of LDS behind the transpose scratch
#define UMNN_BWD_NP(NH) ((NH) < 3 ? 2 : 1)  // points of an element in flight: three hidden layers leave no registers for a second one

struct UmnnBwdArgs {
  const float* x;
  const float* signal;
  const float* image;
  const float* quad;
  const int* feat;
  const float* gy;
  const float* gl;
  float* gx;
  float* gsignal;
  float* work;
  long long N, ldx, lds, ldcol, ldgx, ldgs;
  int Dsel, n_features, rows_per_chunk, gl_reduced, lds_main, n_quad;
  MnnLayout L;
  MnnBwdLayout B;
};

// The helpers below serve NP points of an element at once: one read of a weight fragment feeds the accumulator chains of all of them, and the
// exponentials of one point overlap the matrix instructions of the other.  Sums that meet in one register run over the points in order.

// v = elu(p) for the T tiles of a layer
template <int NP> __device__ __forceinline__ void ubw_act(const mnn_f4 (&p)[NP][MNN_BWD_TM], int T, mnn_f4 (&v)[NP][MNN_BWD_TM]) {
  mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE {
    mnn_for<NP>([&](auto n) MNN_INLINE {
      v[n][o] = bwd_zero();
      if (o < T) {
        mnn_for<4>([&](auto r) MNN_INLINE {
          v[n][o][(int)r] = mnn_elu(p[n][o][(int)r]);
        });
      }
    });
  });
}

// pb = ab elu'(p): elu' is 1 for p > 0 and exp(p) otherwise
template <int NP> __device__ __forceinline__ void ubw_local(const mnn_f4 (&p)[NP][MNN_BWD_TM], int T, const mnn_f4 (&ab)[NP][MNN_BWD_TM], mnn_f4 (&pb)[NP][MNN_BWD_TM]) {
  mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE {
    mnn_for<NP>([&](auto n) MNN_INLINE {
      pb[n][o] = bwd_zero();
      if (o < T) {
        mnn_for<4>([&](auto r) MNN_INLINE {
          float unused, d;
          mnn_elu(p[n][o][(int)r], unused, d);
          pb[n][o][(int)r] = ab[n][o][(int)r] * d;
        });
      }
    });
  });
}

extern __shared__ __attribute__((aligned(16))) float umnn_bwd_lds[];

template <int NH, int TS> __global__ __launch_bounds__(MNN_THREADS, 1) void umnn_bwd_kernel(UmnnBwdArgs a) {
  constexpr int TM = MNN_BWD_TM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
  const MnnLayout& L = a.L;
  const MnnBwdLayout& B = a.B;
  const int col = blockIdx.y;
  const int nq = a.n_quad;
  int f = a.feat ? a.feat[col] : col;
  f = f < 0 ? 0 : (f >= a.n_features ? a.n_features - 1 : f);  // (a memory guard only: the caller checks the range)
  const float* img = a.image + (size_t)f * B.total;
  float* const lds = umnn_bwd_lds;
  float* const scr = umnn_bwd_lds + a.lds_main + wave * MNN_BWD_SCRATCH;
  const float* const qt = umnn_bwd_lds + a.lds_main + (MNN_THREADS / 64) * MNN_BWD_SCRATCH;  // nodes [nq], weights [nq]
  for (int i = tid; i < 2 * nq; i += MNN_THREADS) umnn_bwd_lds[a.lds_main + (MNN_THREADS / 64) * MNN_BWD_SCRATCH + i] = a.quad[i];
  for (int i = tid * 4; i < B.total; i += MNN_THREADS * 4) *reinterpret_cast<mnn_f4*>(lds + i) = *reinterpret_cast<const mnn_f4*>(img + i);
  __syncthreads();

  const int T0 = L.T[0], T1 = L.T[1], T2 = L.T[2], TL = L.T[NH - 1];
  mnn_f4 aW0[TM][TS], aW1[TM][TM], aW2[TM][TM], aX[TM], aB0[TM], aB1[TM], aB2[TM], aWl[TM];
  float aBl = 0.f;
  mnn_for<TM>([&](auto o) MNN_INLINE {
    mnn_for<TS>([&](auto i) MNN_INLINE { aW0[o][i] = bwd_zero(); });
    mnn_for<TM>([&](auto i) MNN_INLINE { aW1[o][i] = bwd_zero(); aW2[o][i] = bwd_zero(); });
    aX[o] = aB0[o] = aB1[o] = aB2[o] = aWl[o] = bwd_zero();
  });

  const long long r0 = (long long)blockIdx.x * a.rows_per_chunk;
  const long long r1 = r0 + a.rows_per_chunk < a.N ? r0 + a.rows_per_chunk : a.N;
  for (long long t0 = r0 + wave * 16; t0 < r1; t0 += (MNN_THREADS / 64) * 16) {
    const long long row = t0 + j;
    const bool valid = row < r1;
    const long long rc = valid ? row : a.N - 1;  // rows behind the end compute on the last row with zero upstream gradients and store nothing
    const float xin = a.x[rc * a.ldx + col];
    const float gyv = (valid && a.gy) ? a.gy[row * a.Dsel + col] : 0.f;
    const float glv = (valid && a.gl) ? (a.gl_reduced ? a.gl[row] : a.gl[row * a.Dsel + col]) : 0.f;

    // ---- the signal's share of the first layer, once per element
    mnn_f4 c0[TM], P0[TM];
    mnn_for<TM>([&](auto o) MNN_INLINE { c0[o] = P0[o] = bwd_zero(); });
    mnn_signal<TM>(L, lds, a.signal + rc * a.lds + (long long)col * a.ldcol, lane, q, c0);

    // ---- the points: the nodes in the order i = 0, 1, ..., then x itself, NP of them per sweep
    float gxv = 0.f;
    auto sweep = [&](auto npc, int k) MNN_INLINE {
      constexpr int NP = decltype(npc)::value;
      bool node[NP];  // (uniform)
      float u[NP];
      mnn_f4 p0[NP][TM], p1[NP][TM], p2[NP][TM], v0[NP][TM], v1[NP][TM], v2[NP][TM];
      mnn_for<NP>([&](auto n) MNN_INLINE {
        node[n] = k + n < nq;
        u[n] = node[n] ? qt[k + n] * xin : xin;
      });
      mnn_for<TM>([&](auto o) MNN_INLINE {
        mnn_for<NP>([&](auto n) MNN_INLINE { p0[n][o] = p1[n][o] = p2[n][o] = bwd_zero(); });
        if (o < T0) {
          const mnn_f4 w = *reinterpret_cast<const mnn_f4*>(lds + L.o_w0x + o * 16 + q * 4);
          mnn_for<NP>([&](auto n) MNN_INLINE {
            mnn_for<4>([&](auto r) MNN_INLINE { p0[n][o][(int)r] = fmaf(w[(int)r], u[n], c0[o][(int)r]); });
          });
        }
      });
      ubw_act<NP>(p0, T0, v0);
      if constexpr (NH > 1) {
        bwd_mv<NP, NP>(lds + L.o_w[1], lds + L.o_b[1], T0, T1, lane, q, v0, p1);
        ubw_act<NP>(p1, T1, v1);
      }
      if constexpr (NH > 2) {
        bwd_mv<NP, NP>(lds + L.o_w[2], lds + L.o_b[2], T1, T2, lane, q, v1, p2);
        ubw_act<NP>(p2, T2, v2);
      }
      const mnn_f4 (&vl)[NP][TM] = NH == 1 ? v0 : (NH == 2 ? v1 : v2);

      // ---- the last layer, the squash and the upstream gradient of h
      mnn_f4 ab[NP][TM], pb[NP][TM];
      mnn_for<NP>([&](auto n) MNN_INLINE {
        float py = 0.f;
        mnn_for<TM>([&](auto o) MNN_INLINE {
          if (o < TL) {
            const mnn_f4 w = *reinterpret_cast<const mnn_f4*>(lds + L.o_wl + o * 16 + q * 4);
            mnn_for<4>([&](auto r) MNN_INLINE { py = fmaf(w[(int)r], vl[n][o][(int)r], py); });
          }
        });
        const float h = mnn_sum_q(py) + lds[L.o_bl];
        const float den = 1.f + fabsf(h / 7.f);
        const float g = expf(h / den);
        const float sqp = 1.f / (den * den);
        const float hb = node[n] ? gyv * xin * qt[nq + k + n] * g * sqp : glv * sqp;
        mnn_for<TM>([&](auto o) MNN_INLINE {
          ab[n][o] = bwd_zero();
          if (o < TL) {
            const mnn_f4 w = *reinterpret_cast<const mnn_f4*>(lds + L.o_wl + o * 16 + q * 4);
            mnn_for<4>([&](auto r) MNN_INLINE {
              ab[n][o][(int)r] = hb * w[(int)r];
              aWl[o][(int)r] += hb * vl[n][o][(int)r];
            });
          }
        });
        if (q == 0) aBl += hb;
        if (!node[n]) gxv = gyv * g;
      });

      // ---- the reverse sweep of these points
      if constexpr (NH > 2) {
        ubw_local<NP>(p2, T2, ab, pb);
        mnn_for<NP>([&](auto n) MNN_INLINE { bwd_add(aB2, pb[n], T2); });
        bwd_outer<NP>(scr, lane, j, q, T2, T1, pb, v1, aW2);
        bwd_mv<NP, 0>(lds + B.o_wT[2], nullptr, T2, T1, lane, q, pb, ab);  // ab = W_2^T pb
      }
      if constexpr (NH > 1) {
        ubw_local<NP>(p1, T1, ab, pb);
        mnn_for<NP>([&](auto n) MNN_INLINE { bwd_add(aB1, pb[n], T1); });
        bwd_outer<NP>(scr, lane, j, q, T1, T0, pb, v0, aW1);
        bwd_mv<NP, 0>(lds + B.o_wT[1], nullptr, T1, T0, lane, q, pb, ab);
      }
      ubw_local<NP>(p0, T0, ab, pb);
      mnn_for<NP>([&](auto n) MNN_INLINE {
        float sx = 0.f;
        mnn_for<TM>([&](auto o) MNN_INLINE {
          if (o < T0) {
            const mnn_f4 w = *reinterpret_cast<const mnn_f4*>(lds + L.o_w0x + o * 16 + q * 4);
            mnn_for<4>([&](auto r) MNN_INLINE {
              aX[o][(int)r] += pb[n][o][(int)r] * u[n];
              P0[o][(int)r] += pb[n][o][(int)r];
              sx = fmaf(w[(int)r], pb[n][o][(int)r], sx);
            });
          }
        });
        if (!node[n]) {
          sx = mnn_sum_q(sx);
          if (a.gx && q == 0 && valid) a.gx[row * a.ldgx + col] = gxv + sx;
        }
      });
    };
    {
      int k = 0;
      if constexpr (UMNN_BWD_NP(NH) > 1)
        for (; k + UMNN_BWD_NP(NH) <= nq + 1; k += UMNN_BWD_NP(NH)) sweep(std::integral_constant<int, UMNN_BWD_NP(NH)>{}, k);
      for (; k <= nq; ++k) sweep(std::integral_constant<int, 1>{}, k);
    }

    // ---- the first layer's bias and signal columns, from the sum over the points
    bwd_add(aB0, P0, T0);
    if (a.work) {  // g W0[:, 1:] += P0 signal^T: the signal of element 4 s + q, feature 16 i + j, read in the operand's own layout
      float PA[TM][4];
      mnn_for<TM>([&](auto o) MNN_INLINE {
        if (o < T0) bwd_transpose(scr, P0[o], lane, j, q, PA[o]);
      });
      mnn_for<TS>([&](auto i) MNN_INLINE {
        if (i < B.ts) {
          const int sidx = i * 16 + j;
          mnn_for<4>([&](auto s) MNN_INLINE {
            const long long er = t0 + s * 4 + q;
            const long long ec = er < a.N ? er : a.N - 1;
            const float b = sidx < L.S ? a.signal[ec * a.lds + (long long)col * a.ldcol + sidx] : 0.f;
            mnn_for<TM>([&](auto o) MNN_INLINE {
              if (o < T0) aW0[o][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(PA[o][s], b, aW0[o][i], 0, 0, 0);
            });
          });
        }
      });
    }
    if (a.gsignal) {
      mnn_for<TS>([&](auto i) MNN_INLINE {
        if (i < B.ts) {
          mnn_f4 gs = bwd_zero();
          mnn_for<TM>([&](auto o) MNN_INLINE {
            if (o < T0) {
              const mnn_f4 a0 = *reinterpret_cast<const mnn_f4*>(lds + B.o_w0sT + (i * T0 + o) * 256 + lane * 4);
              mnn_for<4>([&](auto r) MNN_INLINE { gs = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[(int)r], P0[o][(int)r], gs, 0, 0, 0); });
            }
          });
          if (valid) {
            float* dst = a.gsignal + row * a.ldgs + (size_t)col * L.S;
            mnn_for<4>([&](auto r) MNN_INLINE {
              const int sidx = i * 16 + q * 4 + r;
              if (sidx < L.S) dst[sidx] = gs[(int)r];
            });
          }
        }
      });
    }
  }
  if (!a.work) return;  // (uniform over the grid: nobody asked for parameter gradients)

  // ---- the block's four waves, added in the order 0, 1, 2, 3 over the LDS the image occupied
  float* const G = lds;
  for (int w = 0; w < MNN_THREADS / 64; ++w) {
    __syncthreads();
    if (wave == w) {
      const bool set = w == 0;
      bwd_put_tiles<TS>(G + B.g_w0s, aW0, T0, B.ts, lane, set);
      bwd_put_units(G + B.g_w0x, aX, T0, j, q, set);
      bwd_put_units(G + B.g_b0, aB0, T0, j, q, set);
      if constexpr (NH > 1) {
        bwd_put_tiles<TM>(G + B.g_w[1], aW1, T1, T0, lane, set);
        bwd_put_units(G + B.g_b[1], aB1, T1, j, q, set);
      }
      if constexpr (NH > 2) {
        bwd_put_tiles<TM>(G + B.g_w[2], aW2, T2, T1, lane, set);
        bwd_put_units(G + B.g_b[2], aB2, T2, j, q, set);
      }
      bwd_put_units(G + B.g_wl, aWl, TL, j, q, set);
      bwd_put_scalar(G + B.g_bl, aBl, lane, set);
    }
  }
  __syncthreads();
  float* out = a.work + ((size_t)blockIdx.x * a.Dsel + col) * B.g_total;
  for (int i = tid * 4; i < B.g_total; i += MNN_THREADS * 4) *reinterpret_cast<mnn_f4*>(out + i) = *reinterpret_cast<const mnn_f4*>(G + i);
}

template <int NH> static const void* umnn_bwd_fn(int ts) {
  if (ts <= 1) return (const void*)umnn_bwd_kernel<NH, 1>;
  if (ts <= 2) return (const void*)umnn_bwd_kernel<NH, 2>;
  return (const void*)umnn_bwd_kernel<NH, 4>;
}

static int umnn_backward(const zk_umnn_bwd_args_v1* p, void* stream) {
  if (!p || p->struct_size != sizeof(zk_umnn_bwd_args_v1) || p->version != 1) return ZK_EINVAL;
  UmnnBwdArgs a;
  if (!mnn_bwd_shape(p->S, p->n_hidden, p->width0, p->width1, p->width2, &a.L, &a.B, 2 * UMNN_QUAD_MAX)) return ZK_EINVAL;
  if (p->image_floats != a.B.total || p->grad_floats != a.B.g_total || p->n_features < 1 || p->N < 0 || p->Dsel < 1 || p->Dsel > 65535) return ZK_EINVAL;
  if (p->n_quad < 1 || p->n_quad > UMNN_QUAD_MAX) return ZK_EINVAL;
  if (p->ldx < 1 || p->ld_col < p->S || p->ld_signal < (p->Dsel - 1) * p->ld_col + p->S) return ZK_EINVAL;
  if (p->gx && p->ld_gx < p->Dsel) return ZK_EINVAL;
  if (p->gsignal && p->ld_gsignal < p->Dsel * (int64_t)p->S) return ZK_EINVAL;
  if (p->gparams && (p->flat_total < 1 || p->flat_weights < 0 || p->flat_weights > p->flat_total)) return ZK_EINVAL;
  if (p->gparams && p->N > 0 && (!p->grad_table || !p->work)) return ZK_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (p->N == 0) {
    if (p->gparams && hipMemsetAsync(p->gparams, 0, (size_t)p->flat_total * 4, st) != hipSuccess) return ZK_LAUNCH_CHECK();
    return 0;
  }
  if (!p->x || !p->signal || !p->image || !p->quad) return ZK_EINVAL;
  int chunks = 0;
  if (mnn_bwd_geometry(p->N, p->Dsel, MNN_BWD_BLOCKS, &a.rows_per_chunk, &chunks) != 0) return ZK_EINVAL;
  a.x = (const float*)p->x; a.signal = (const float*)p->signal; a.image = (const float*)p->image; a.quad = (const float*)p->quad; a.feat = (const int*)p->feat;
  a.gy = (const float*)p->gy; a.gl = (const float*)p->gl; a.gx = (float*)p->gx; a.gsignal = (float*)p->gsignal;
  a.work = p->gparams ? (float*)p->work : nullptr;
  a.N = p->N; a.ldx = p->ldx; a.lds = p->ld_signal; a.ldcol = p->ld_col; a.ldgx = p->ld_gx; a.ldgs = p->ld_gsignal;
  a.Dsel = (int)p->Dsel; a.n_features = p->n_features; a.gl_reduced = p->gl_reduced; a.n_quad = p->n_quad;
  a.lds_main = a.B.total > a.B.g_total ? a.B.total : a.B.g_total;
  if (p->gparams && hipMemsetAsync(p->gparams, 0, (size_t)p->flat_total * 4, st) != hipSuccess) return ZK_LAUNCH_CHECK();
  if (!a.gx && !a.gsignal && !a.work) return 0;
  const void* fn = a.L.nh == 1 ? umnn_bwd_fn<1>(a.B.ts) : (a.L.nh == 2 ? umnn_bwd_fn<2>(a.B.ts) : umnn_bwd_fn<3>(a.B.ts));
  const int rc = mnn_launch_dyn_lds(fn, dim3((unsigned)chunks, (unsigned)a.Dsel), (mnn_bwd_lds_floats(a.B) + 2 * UMNN_QUAD_MAX) * 4, &a, st);
  if (rc != 0 || !a.work) return rc;
  return mnn_bwd_reduce((const float*)a.work, (const int*)p->grad_table, a.feat, nullptr, (float*)p->gparams, chunks, a.Dsel, a.B.g_total, a.n_features,
                        (long long)p->flat_weights, (long long)p->flat_total, false, st);
}

}  // namespace zk

extern "C" int zk_umnn_backward(const zk_umnn_bwd_args_v1* args, void* stream) { return zk::umnn_backward(args, stream); }
extern "C" int zk_umnn_backward_geometry(int64_t N, int64_t Dsel, int* rows_per_chunk, int* n_chunks) {
  return zk::mnn_bwd_geometry(N, Dsel, MNN_BWD_BLOCKS, rows_per_chunk, n_chunks);
}
extern "C" int zk_umnn_backward_floats(int S, int n_hidden, int width0, int width1, int width2, int* image_floats, int* grad_floats) {
  return zk::mnn_bwd_floats<2 * UMNN_QUAD_MAX>(S, n_hidden, width0, width1, width2, image_floats, grad_floats);
}
extern "C" int zk_umnn_backward_workspace_floats(int64_t N, int64_t Dsel, int S, int n_hidden, int width0, int width1, int width2, int64_t* floats) {
  return zk::mnn_bwd_workspace_floats<2 * UMNN_QUAD_MAX>(N, Dsel, S, n_hidden, width0, width1, width2, floats);
}
