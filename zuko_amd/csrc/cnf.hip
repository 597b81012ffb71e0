// zuko_amd — continuous normalizing flow (CNF): one attempted Dormand-Prince 5(4) step of the free-form Jacobian ODE for all rows.
//
// Replaces one pass of the inner loop of AdaptiveCheckpointAdjoint.forward (zuko/utils.py:515-554): dopri45(f_aug, (x, ladj), t, dt, error=True)
// with f_aug of FreeFormJacobianTransform.call_and_ladj (zuko/transforms.py:1147-1179) and f of FFJTransform (zuko/flows/continuous.py:88-97),
// and the per-row share of max(error / tolerance).  The reference runs seven MLP evaluations, each with a batched autograd Jacobian (`features`
// backward passes under vmap) for the trace: several hundred launches per attempt.  Here it is one.
//
// Execution model (gfx950):
//   * a wavefront owns 16 rows for the whole step.  As in csrc/mnn.hip every layer is computed transposed, H^T = W X^T, on
//     v_mfma_f32_16x16x4_f32 (exact fp32): the 16 columns of a tile are the wave's 16 rows, lane (j, q) = (lane & 15, lane >> 4) of a D fragment
//     holds out units 16 t + 4 q + r (r = 0..3) of row j, which is the next layer's B operand with the weight image laid out in that k order.
//   * the state lives in registers in the SAME distribution: lane (j, q) holds features 4 s + q (slots s = 0..3) of row j — the B operand of the
//     first layer's x product as it stands — and the last layer's rows are permuted in the image so that its D fragment comes out in that
//     distribution too.  The seven k vectors are 4 registers each per lane; the log-determinant's k and the row's l are kept in all four lanes.
//   * the exact trace is carried in forward mode: the value pass keeps act'(pre) of every hidden layer (D_l); tangent i enters as D_1 o W0x[:, i],
//     goes through the hidden layers on the same A fragments (two tangents at a time for networks up to 64 wide: four independent accumulator
//     chains per fragment read), and meets row i of the last layer in a per-lane dot product and two cross-lane adds: only the diagonal of the
//     last product is formed.  The trace adds the tangents' terms in the order i = 0, 1, ...
//   * the stage loop is a run-time loop over one body (seven unrolled bodies would not fit the instruction cache): the Butcher rows come from a
//     table, zero entries included — adding 0 * k changes nothing, so the sums are the reference's left to right.
//   * the weight image (zuko_amd/cnf_plan.py: layout) sits in LDS, shared by the block's 4 wavefronts; a block covers 64 rows.
//   * the error ratio is reduced per row over the four lanes, per wave over the rows, and one lane per wave joins an integer atomic maximum on
//     the bits of |ratio| (NaN > inf > finite in that order): the one float the host reads back per attempt.
//
// A row's outputs depend on its own x, l and pre row only: not on N, the launch geometry or its neighbours.
#include "zk_cnf_common.h"

namespace zk {

#define CNF_ROWS 64  // rows per block: one 16-row tile per wavefront

// (the image's layout CnfLayout, the Dormand-Prince tableau CNF_C / CNF_A / CNF_E, the time embedding and the first layer's pre-activation:
//  csrc/zk_cnf_common.h, shared with the adjoint kernel of csrc/cnf_backward.hip; the paired layer product mnn_matvec and the activation mnn_elu:
//  csrc/zk_mnn_common.h)
struct CnfArgs {
  const float* x;
  const float* l;
  const float* pre;
  const float* image;
  const float* eps;
  float* y;
  float* l_next;
  unsigned* err;
  float* err_rows;
  long long N, ldx, ldy, ld_pre, ld_eps;
  float t, dt, atol, rtol, tscale;
  CnfLayout L;
};

// max that keeps a NaN from either side (torch.max does; fmaxf drops it)
__device__ __forceinline__ float cnf_max(float a, float b) { return (a > b || a != a) ? a : b; }

// v = ELU(p) and, with TAN, D = ELU'(p) of one tile
template <bool TAN> __device__ __forceinline__ void cnf_elu_tile(const mnn_f4& p, mnn_f4& v, mnn_f4& D) {
  mnn_for<4>([&](auto r) MNN_INLINE {
    if constexpr (TAN) {
      float av, ad;
      mnn_elu(p[(int)r], av, ad);
      v[(int)r] = av;
      D[(int)r] = ad;
    } else {
      v[(int)r] = mnn_elu(p[(int)r]);
    }
  });
}

// G tangents i0 .. i0 + G - 1 through the network behind the first layer's pre-activation: returns W_last[i, :] T[:, i] summed over them in order
template <int TM, int G>
__device__ __forceinline__ float cnf_tangents(const CnfLayout& L, const float* lds, int lane, int q, int i0, const mnn_f4 (&D)[3][TM]) {
  mnn_f4 a[G][TM], b[G][TM];
  const int H0 = L.T[0] * 16;
  mnn_for<G>([&](auto g) MNN_INLINE {
    mnn_for<TM>([&](auto o) MNN_INLINE {
      if (o < L.T[0]) {
        const mnn_f4 w = *reinterpret_cast<const mnn_f4*>(lds + L.o_w0c + (i0 + g) * H0 + o * 16 + q * 4);
        mnn_for<4>([&](auto r) MNN_INLINE { a[g][o][(int)r] = D[0][o][(int)r] * w[(int)r]; });
      }
    });
  });
  if (L.nh > 1) {
    mnn_matvec<TM, G, 0>(lds + L.o_w[1], nullptr, L.T[0], L.T[1], lane, q, a, b);
    mnn_for<G>([&](auto g) MNN_INLINE {
      mnn_for<TM>([&](auto o) MNN_INLINE {
        if (o < L.T[1]) mnn_for<4>([&](auto r) MNN_INLINE { a[g][o][(int)r] = D[1][o][(int)r] * b[g][o][(int)r]; });
      });
    });
  }
  if (L.nh > 2) {
    mnn_matvec<TM, G, 0>(lds + L.o_w[2], nullptr, L.T[1], L.T[2], lane, q, a, b);
    mnn_for<G>([&](auto g) MNN_INLINE {
      mnn_for<TM>([&](auto o) MNN_INLINE {
        if (o < L.T[2]) mnn_for<4>([&](auto r) MNN_INLINE { a[g][o][(int)r] = D[2][o][(int)r] * b[g][o][(int)r]; });
      });
    });
  }
  const int tl = L.T[L.nh - 1];
  float tr = 0.f;
  mnn_for<G>([&](auto g) MNN_INLINE {
    float p = 0.f;
    mnn_for<TM>([&](auto o) MNN_INLINE {
      if (o < tl) {
        const mnn_f4 w = *reinterpret_cast<const mnn_f4*>(lds + L.o_wl + (i0 + g) * tl * 16 + o * 16 + q * 4);
        mnn_for<4>([&](auto r) MNN_INLINE { p = fmaf(w[(int)r], a[g][o][(int)r], p); });
      }
    });
    tr += mnn_sum_q(p);
  });
  return tr;
}

// Hutchinson's estimate of the trace, ep^T (df/dx) ep, of the wave's rows: ONE tangent in direction ep (held as the state is: lane (j, q), features
// 4 s + q, zero behind F).  Z_1 = W0x ep is the x part of cnf_first_layer, the hidden layers are those of one member of cnf_tangents, and the last
// layer's product is the field's with a zero accumulator: u = W_last T_L comes out in the state's distribution and meets ep in four per-lane products.
template <int TM>
__device__ __forceinline__ float cnf_probe(const CnfLayout& L, const float* lds, int lane, int q, const float (&ep)[4], const mnn_f4 (&D)[3][TM]) {
  mnn_f4 a[TM], b[TM];
  const float* const px = lds + L.o_w0x + lane;
  mnn_for<TM>([&](auto o) MNN_INLINE {
    if (o < L.T[0]) {
      mnn_f4 z = {0.f, 0.f, 0.f, 0.f};
      mnn_for<4>([&](auto s) MNN_INLINE {
        if (s < L.kx) z = __builtin_amdgcn_mfma_f32_16x16x4f32(px[(o * L.kx + s) * 64], ep[s], z, 0, 0, 0);
      });
      mnn_for<4>([&](auto r) MNN_INLINE { a[o][(int)r] = D[0][o][(int)r] * z[(int)r]; });
    }
  });
  if (L.nh > 1) {
    mnn_matvec<TM, 1, 0>(lds + L.o_w[1], nullptr, L.T[0], L.T[1], lane, q, &a, &b);
    mnn_for<TM>([&](auto o) MNN_INLINE {
      if (o < L.T[1]) mnn_for<4>([&](auto r) MNN_INLINE { a[o][(int)r] = D[1][o][(int)r] * b[o][(int)r]; });
    });
  }
  if (L.nh > 2) {
    mnn_matvec<TM, 1, 0>(lds + L.o_w[2], nullptr, L.T[1], L.T[2], lane, q, &a, &b);
    mnn_for<TM>([&](auto o) MNN_INLINE {
      if (o < L.T[2]) mnn_for<4>([&](auto r) MNN_INLINE { a[o][(int)r] = D[2][o][(int)r] * b[o][(int)r]; });
    });
  }
  const int tl = L.T[L.nh - 1];
  mnn_f4 u = {0.f, 0.f, 0.f, 0.f};
  mnn_for<TM>([&](auto it) MNN_INLINE {
    if (it < tl) {
      const mnn_f4 w = *reinterpret_cast<const mnn_f4*>(lds + L.o_wo + it * 256 + lane * 4);
      mnn_for<4>([&](auto r) MNN_INLINE { u = __builtin_amdgcn_mfma_f32_16x16x4f32(w[(int)r], a[it][(int)r], u, 0, 0, 0); });
    }
  });
  float p = 0.f;
  mnn_for<4>([&](auto s) MNN_INLINE { p = fmaf(ep[s], u[(int)s], p); });
  return mnn_sum_q(p);
}

// f(ts, xin) of the wave's 16 rows: fo[r] = component 4 r + q of the field, tr = the trace of its Jacobian (TAN), or its estimate along ep (PROBE)
template <int TM, bool TAN, bool PROBE>
__device__ __forceinline__ void cnf_field(const CnfLayout& L, const float* lds, const float* __restrict__ prow, int lane, int q, float ts, const float (&xin)[4],
                                          const float (&ep)[4], float (&fo)[4], float& tr) {
  mnn_f4 v[TM], w[TM], D[3][TM];
  float emb[4];
  mnn_for<4>([&](auto s) MNN_INLINE {
    emb[s] = 0.f;
    if (s < L.kt) emb[s] = cnf_embed(L, lds, 4 * s + q, ts);
  });
  mnn_for<TM>([&](auto o) MNN_INLINE {
    if (o < L.T[0]) cnf_elu_tile<TAN>(cnf_first_layer(L, lds, prow, lane, q, o, emb, xin), v[o], D[0][o]);
  });
  if (L.nh > 1) {
    mnn_matvec<TM, 1, 1>(lds + L.o_w[1], lds + L.o_b[1], L.T[0], L.T[1], lane, q, &v, &w);
    mnn_for<TM>([&](auto o) MNN_INLINE {
      if (o < L.T[1]) cnf_elu_tile<TAN>(w[o], v[o], D[1][o]);
    });
  }
  if (L.nh > 2) {
    mnn_matvec<TM, 1, 1>(lds + L.o_w[2], lds + L.o_b[2], L.T[1], L.T[2], lane, q, &v, &w);
    mnn_for<TM>([&](auto o) MNN_INLINE {
      if (o < L.T[2]) cnf_elu_tile<TAN>(w[o], v[o], D[2][o]);
    });
  }
  // last layer: its rows are stored so that register r of lane (j, q) is feature 4 r + q
  const int tl = L.T[L.nh - 1];
  mnn_f4 c = *reinterpret_cast<const mnn_f4*>(lds + L.o_bo + q * 4);
  mnn_for<TM>([&](auto it) MNN_INLINE {
    if (it < tl) {
      const mnn_f4 a = *reinterpret_cast<const mnn_f4*>(lds + L.o_wo + it * 256 + lane * 4);
      mnn_for<4>([&](auto r) MNN_INLINE { c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[(int)r], v[it][(int)r], c, 0, 0, 0); });
    }
  });
  mnn_for<4>([&](auto r) MNN_INLINE { fo[r] = c[(int)r]; });
  if constexpr (PROBE) {
    tr = cnf_probe<TM>(L, lds, lane, q, ep, D);
  } else if constexpr (TAN) {
    tr = 0.f;
    int i = 0;
    if constexpr (TM <= 4) {
      for (; i + 2 <= L.F; i += 2) tr += cnf_tangents<TM, 2>(L, lds, lane, q, i, D);
    }
    for (; i < L.F; ++i) tr += cnf_tangents<TM, 1>(L, lds, lane, q, i, D);
  }
}

extern __shared__ __attribute__((aligned(16))) float cnf_lds[];

// TAN: the state carries l; its trace is exact (one tangent per feature) or, with PROBE (which implies TAN), Hutchinson's estimate along the row's eps
template <int TM, bool TAN, bool PROBE = false> __global__ __launch_bounds__(MNN_THREADS, TM <= 4 ? 2 : 1) void cnf_step_kernel(CnfArgs a) {
  static_assert(TAN || !PROBE);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
  const CnfLayout& L = a.L;
  mnn_stage_image(cnf_lds, a.image, L.total, tid);
  __syncthreads();
  const long long row0 = (long long)blockIdx.x * CNF_ROWS + wave * 16;
  if (row0 >= a.N) return;  // (the whole wavefront; no barrier follows)
  const long long row = row0 + j;
  const long long rc = row < a.N ? row : a.N - 1;  // rows behind the end compute on the last row and store nothing
  const float* const prow = a.pre + rc * a.ld_pre;
  float x[4], xs[4], xn[4], k[7][4], kl[7];
  mnn_for<4>([&](auto s) MNN_INLINE { x[s] = 4 * s + q < L.F ? a.x[rc * a.ldx + 4 * s + q] : 0.f; });
  float l0 = 0.f, ln = 0.f, ep[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (TAN) l0 = a.l[rc];
  if constexpr (PROBE) mnn_for<4>([&](auto s) MNN_INLINE { ep[s] = 4 * s + q < L.F ? a.eps[rc * a.ld_eps + 4 * s + q] : 0.f; });
  mnn_for<7>([&](auto m) MNN_INLINE {
    kl[m] = 0.f;
    mnn_for<4>([&](auto s) MNN_INLINE { k[m][s] = 0.f; });
  });
#pragma unroll 1
  for (int s = 0; s < 7; ++s) {
    // x + A[s][0] k1 + A[s][1] k2 + ..., left to right (a zero entry adds nothing)
    mnn_for<4>([&](auto c) MNN_INLINE {
      float acc = x[c];
      mnn_for<6>([&](auto m) MNN_INLINE { acc = acc + CNF_A[s][m] * k[m][c]; });
      xs[c] = acc;
    });
    if (s == 6) {
      mnn_for<4>([&](auto c) MNN_INLINE { xn[c] = xs[c]; });
      if constexpr (TAN) {
        float acc = l0;
        mnn_for<6>([&](auto m) MNN_INLINE { acc = acc + CNF_A[6][m] * kl[m]; });
        ln = acc;
      }
    }
    const float ts = a.t + CNF_C[s] * a.dt;
    float fo[4], tr = 0.f;
    cnf_field<TM, TAN, PROBE>(L, cnf_lds, prow, lane, q, ts, xs, ep, fo, tr);
    mnn_for<7>([&](auto m) MNN_INLINE {
      if (s == m) {
        mnn_for<4>([&](auto c) MNN_INLINE { k[m][c] = a.dt * fo[c]; });
        if constexpr (TAN) kl[m] = a.dt * (tr * a.tscale);
      }
    });
  }
  // next - star of the embedded pair and the ratio |next - star| / (atol + rtol max(|state|, |next|))
  float ratio = 0.f;
  mnn_for<4>([&](auto c) MNN_INLINE {
    float diff = CNF_E[0] * k[0][c];
    mnn_for<7>([&](auto m) MNN_INLINE {
      if (m > 1) diff = diff + CNF_E[m] * k[m][c];
    });
    const float tol = a.atol + a.rtol * cnf_max(fabsf(x[c]), fabsf(xn[c]));
    const float rt = fabsf(diff) / tol;
    if (4 * c + q < L.F) ratio = cnf_max(ratio, rt);
  });
  if constexpr (TAN) {
    float diff = CNF_E[0] * kl[0];
    mnn_for<7>([&](auto m) MNN_INLINE {
      if (m > 1) diff = diff + CNF_E[m] * kl[m];
    });
    const float tol = a.atol + a.rtol * cnf_max(fabsf(l0), fabsf(ln));
    ratio = cnf_max(ratio, fabsf(diff) / tol);
  }
  ratio = cnf_max(ratio, __shfl_xor(ratio, 16, 64));
  ratio = cnf_max(ratio, __shfl_xor(ratio, 32, 64));
  if (row < a.N) {
    mnn_for<4>([&](auto c) MNN_INLINE {
      if (4 * c + q < L.F) a.y[row * a.ldy + 4 * c + q] = xn[c];
    });
    if (q == 0) {
      if constexpr (TAN) a.l_next[row] = ln;
      if (a.err_rows) a.err_rows[row] = ratio;
    }
  }
  unsigned bits = row < a.N ? (__float_as_uint(ratio) & 0x7fffffffu) : 0u;
  for (int off = 1; off < 16; off <<= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)bits, off, 64);
    bits = o > bits ? o : bits;
  }
  if (lane == 0) atomicMax(a.err, bits);
}

// the launcher of both argument blocks: P is zk_cnf_args_v1 (eps = NULL) or zk_cnf_args_v2, whose first fields are v1's
template <class P> static int cnf_step(const P* p, uint32_t version, const void* eps, long long ld_eps, void* stream) {
  if (!p || p->struct_size != sizeof(P) || p->version != version) return ZK_EINVAL;
  CnfArgs a;
  const int widths[3] = {p->width0, p->width1, p->width2};
  if (!cnf_layout(p->features, p->freqs, p->n_hidden, widths, &a.L)) return ZK_EINVAL;
  if (p->image_floats != a.L.total || (p->n_tangents != 0 && p->n_tangents != p->features) || p->N < 0) return ZK_EINVAL;
  if (p->ldx < p->features || p->ldy < p->features) return ZK_EINVAL;
  if (!cnf_step_fields_ok(p, p->n_tangents != 0)) return ZK_EINVAL;
  if (!(p->atol >= 0) || !(p->rtol >= 0) || !std::isfinite(p->atol) || !std::isfinite(p->rtol)) return ZK_EINVAL;
  if (p->N == 0) return 0;
  if (!p->x || !p->pre || !p->image || !p->y || !p->err) return ZK_EINVAL;
  if (p->n_tangents != 0 && (!p->l || !p->l_next)) return ZK_EINVAL;
  if (eps && (p->n_tangents == 0 || ld_eps < p->features)) return ZK_EINVAL;  // the estimator belongs to a traced call
  if (((uintptr_t)p->pre | (uintptr_t)p->image) % 16 != 0) return ZK_EINVAL;
  const long long gx = (p->N + CNF_ROWS - 1) / CNF_ROWS;
  if (gx > 0x7fffffffLL) return ZK_EINVAL;
  a.x = (const float*)p->x; a.l = (const float*)p->l; a.pre = (const float*)p->pre; a.image = (const float*)p->image; a.eps = (const float*)eps;
  a.y = (float*)p->y; a.l_next = (float*)p->l_next; a.err = (unsigned*)p->err; a.err_rows = (float*)p->err_rows;
  a.N = p->N; a.ldx = p->ldx; a.ldy = p->ldy; a.ld_pre = p->ld_pre; a.ld_eps = ld_eps;
  a.t = (float)p->t; a.dt = (float)p->dt; a.atol = (float)p->atol; a.rtol = (float)p->rtol; a.tscale = (float)p->trace_scale;
  const bool small = a.L.T[0] <= 4 && a.L.T[1] <= 4 && a.L.T[2] <= 4;
  const bool tan = p->n_tangents != 0;
  const void* fn = eps ? (small ? (const void*)cnf_step_kernel<4, true, true> : (const void*)cnf_step_kernel<8, true, true>)
                 : small ? (tan ? (const void*)cnf_step_kernel<4, true> : (const void*)cnf_step_kernel<4, false>)
                         : (tan ? (const void*)cnf_step_kernel<8, true> : (const void*)cnf_step_kernel<8, false>);
  return mnn_launch_dyn_lds(fn, dim3((unsigned)gx), a.L.total * 4, &a, (hipStream_t)stream);
}

}  // namespace zk

extern "C" int zk_cnf_step(const zk_cnf_args_v1* args, void* stream) { return zk::cnf_step(args, 1, nullptr, 0, stream); }
extern "C" int zk_cnf_step_v2(const zk_cnf_args_v2* args, void* stream) {
  return zk::cnf_step(args, 2, args ? args->eps : nullptr, args ? (long long)args->ld_eps : 0, stream);
}
extern "C" int zk_cnf_image_floats(int features, int freqs, int n_hidden, int width0, int width1, int width2) {
  zk::CnfLayout L;
  const int widths[3] = {width0, width1, width2};
  return zk::cnf_layout(features, freqs, n_hidden, widths, &L) ? L.total : -1;
}
