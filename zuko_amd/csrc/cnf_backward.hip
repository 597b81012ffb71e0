// zuko_amd — adjoint of the continuous normalizing flow (CNF): ONE reverse Dormand-Prince step of the augmented system (x, a, g_phi) for all rows.
//
// Replaces one pass of the loop of AdaptiveCheckpointAdjoint.backward (zuko/utils.py:556-593) over the stored accepted steps: a six-stage step of size
// h = -dt from the checkpoint AFTER the forward step, no error estimate, nothing read back.  With beta = al * trace_scale (al: the adjoint of the
// log-determinant component, constant along the integration) stage s evaluates, at t_s = t + c_s h on (x_s, a_s),
//     kx_s = h f(t_s, x_s)        ka_s = dt (a_s^T df/dx + beta d trace/dx)
// and adds  b_s dt (a_s^T df/dphi + beta d trace/dphi)  to every parameter gradient (b: the fifth-order weights): the parameter components never
// feed a stage input, so their accumulators run across the six stages with the stage's cotangents scaled by sigma_s = b_s dt.
//
// The reverse sweep of one stage, with p_l the pre-activations, h_l = ELU(p_l), D_l = ELU'(p_l), D'_l = ELU''(p_l) = (p_l > 0 ? 0 : D_l):
//   value  hb_L = W_last^T a,   pb_l = D_l o hb_l + Db_l o D'_l,   hb_{l-1} = W_l^T pb_l
//   trace  per feature i, forward  T_1 = D_1 o W0x[:, i], Z_{l+1} = W_{l+1} T_l, T_{l+1} = D_{l+1} o Z_{l+1}   (Z_1 = W0x[:, i])
//          reverse  Tb_L = beta W_last[i, :],  Db_l += Tb_l o Z_l,  Zb_l = Tb_l o D_l,  Tb_{l-1} = W_l^T Zb_l
//          g W_last[i, :] += beta T_L,   g W_l += Zb_l T_{l-1}^T,   g W0x[:, i] += Tb_1 o D_1
//   out    a^T df/dx + beta d trace/dx = W0x^T pb_1,   g W_l += pb_l h_{l-1}^T,  g b_l += pb_l,  g W0x += pb_1 x^T,  g W0t += pb_1 emb(t_s)^T,
//          g pre += pb_1,   g W_last += a h_L^T,  g b_last += a
// The trace terms of Db_l join pb_l before it is pulled through W_l^T, so a stage runs in two passes: the value forward (keeping D_l), the loop
// over the features (one tangent forward and back at a time, accumulating Db_l), then the value forward AGAIN for h_l — cheaper than holding
// 48 more registers across the feature loop — and the value reverse.
//
// Execution model (gfx950), that of csrc/cnf.hip and csrc/mnn_backward.hip:
//   * a wavefront owns 16 rows; every product is transposed, on v_mfma_f32_16x16x4_f32 (exact fp32); lane (j, q) = (lane & 15, lane >> 4) holds
//     units 16 o + 4 q + r of row j (the D fragment), and the states x, a and their k vectors as features 4 s + q (slots s = 0..3) of row j.
//   * the BACKWARD image sits in LDS: the forward image followed by the transposed tiles (zuko_amd/cnf_plan.py: layout_backward), so that every
//     W^T product is a forward product with the roles of `in` and `out` exchanged.
//   * weight gradients contract over the wave's 16 rows: both operands go through 256 floats of per-wave LDS (bwd_transpose of
//     csrc/zk_mnn_bwd_common.h); the accumulators of every weight stay in registers across the stages and the block's row tiles — one wavefront per
//     SIMD.  Terms that are a column of a weight per feature (g W_last[i, :], g W0x[:, i]) are added over the 16 row lanes and kept by lane j = i.
//   * what would not fit 512 registers at three layers of 64 lives elsewhere: the stages' k vectors and the launch's g pre sum in a per-wave slice
//     of the workspace (a lane reads back only what it wrote), the bias gradients and, per stage, the rows' sum of pb_1 (g W0t = that sum times
//     emb(t_s)^T, formed once at the end) in CNF_ADJ_COLS floats of LDS per wave; x and ax are read again where a sum starts from them.
//   * a block covers one row chunk (zk_cnf_adjoint_geometry); its four waves are added in LDS in the order 0, 1, 2, 3 and ONE partial per chunk
//     goes to `work`; cnf_adj_reduce_kernel adds the partials in chunk order INTO gparams through the gradient table.  No atomics: the same inputs
//     give the same bits.  gpre is accumulated by the lane that owns the element (read, add, write).
// A row's ax_next and gpre depend on its own x, ax, al and pre row only.
#include "zk_cnf_common.h"
#include "zk_mnn_bwd_common.h"

namespace zk {

#define CNF_ADJ_BLOCKS 256  // the grid aims at this many blocks: one per CU (one wavefront per SIMD)
#define CNF_ADJ_COLS 512    // floats of column sums per wavefront: g b_1, g b_2 (64 each) and, per stage, the rows' sum of sigma pb_1 (6 x 64)
#define CNF_ADJ_KVECS (6 * 2 * 4 * 64)       // floats of k vectors per 16-row tile: six stages of (kx, ka), four slots, 64 lanes
#define CNF_ADJ_KTILE (CNF_ADJ_KVECS + 1024)  // floats of scratch per 16-row tile: the k vectors and the launch's g pre (4 tiles x 64 lanes x 4)

// Offsets (floats) behind the forward image, and of one row chunk's partial; the arithmetic of zuko_amd/cnf_plan.py: layout_backward.
struct CnfAdjLayout {
  int o_wT[3];  // l = 1, 2: [T_{l-1}][T_l][256], lane (j, q), r of tile (i, o): W_l[16 o + 4 q + r][16 i + j]
  int o_woT;    // [T_last][kx][64], lane (j, q) of tile o, k-step s: W_last[4 s + q][16 o + j] (zero behind F)
  int o_w0xT;   // [T_0][256], lane (j, q), r of tile i: W0x[16 i + 4 q + r][feature 4 (j & 3) + (j >> 2)] (zero behind F)
  int total;    // the backward image
  int g_w0t, g_w0x, g_w[3], g_b[3], g_wo, g_bo, g_total;
};

static inline bool cnf_adj_layout(const CnfLayout& L, CnfAdjLayout* B) {
  for (int l = 0; l < L.nh; ++l)
    if (L.T[l] > MNN_BWD_TM) return false;
  int o = L.total;
  B->o_wT[0] = 0;
  for (int l = 1; l < 3; ++l) {
    B->o_wT[l] = o;
    if (l < L.nh) o += L.T[l] * L.T[l - 1] * 256;
  }
  B->o_woT = o; o += L.T[L.nh - 1] * L.kx * 64;
  B->o_w0xT = o; o += L.T[0] * 256;
  B->total = o;
  int g = 0;
  B->g_w0t = g; g += L.T[0] * 256;
  B->g_w0x = g; g += L.T[0] * 256;
  B->g_w[0] = B->g_b[0] = 0;
  for (int l = 1; l < 3; ++l) {
    B->g_w[l] = g; if (l < L.nh) g += L.T[l] * L.T[l - 1] * 256;
    B->g_b[l] = g; if (l < L.nh) g += L.T[l] * 16;
  }
  B->g_wo = g; g += L.T[L.nh - 1] * 256;
  B->g_bo = g; g += 16;
  B->g_total = g;
  return true;
}

static inline int cnf_adj_lds_floats(const CnfAdjLayout& B) { return (B.total > B.g_total ? B.total : B.g_total) + (MNN_THREADS / 64) * (MNN_BWD_SCRATCH + CNF_ADJ_COLS); }

static inline bool cnf_adj_shape(int F, int Q, int nh, int w0, int w1, int w2, CnfLayout* L, CnfAdjLayout* B) {
  const int widths[3] = {w0, w1, w2};
  if (!cnf_layout(F, Q, nh, widths, L)) return false;
  if (!cnf_adj_layout(*L, B)) return false;
  return cnf_adj_lds_floats(*B) * 4 <= MNN_LDS_MAX;
}

struct CnfAdjArgs {
  const float* x;
  const float* ax;
  const float* al;
  const float* pre;
  const float* image;
  const float* eps;
  float* ax_next;
  float* gpre;
  float* work;
  float* kbuf;
  long long N, ldx, ldax, ldan, ld_pre, ld_gpre, ld_eps;
  int rows_per_chunk, lds_main;
  float t, dt, tscale;
  CnfLayout L;
  CnfAdjLayout B;
};

// out = W in (+ b): tiles [tout][tin][256] of the image — a forward product, or a transposed one through the transposed tiles.  bwd_mv<1, NB> of
// csrc/zk_mnn_bwd_common.h without the run-time test of `Bias`: kept, because cnf_adj_kernel<3, true> takes 507 registers with that one and 506 with
// this (profiles/small_net_frame/census.md)
__device__ __forceinline__ void adj_mv(const float* W, const float* Bias, int tin, int tout, int lane, int q, bwd_ctiles in, bwd_tiles out) {
  mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE {
    out[o] = bwd_zero();
    if (o < tout) {
      if (Bias) out[o] = *reinterpret_cast<const mnn_f4*>(Bias + o * 16 + q * 4);
      mnn_for<MNN_BWD_TM>([&](auto it) MNN_INLINE {
        if (it < tin) {
          const mnn_f4 a0 = *reinterpret_cast<const mnn_f4*>(W + (o * tin + it) * 256 + lane * 4);
          mnn_for<4>([&](auto r) MNN_INLINE { out[o] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[(int)r], in[it][(int)r], out[o], 0, 0, 0); });
        }
      });
    }
  });
}

// A state held as (row j, features 4 s + q) becomes the four k-steps of a B operand that contracts over the rows: out[s] = state[row 4 s + q][feature j]
__device__ __forceinline__ void adj_state_transpose(float* scr, const float (&v)[4], int lane, int j, int q, float (&out)[4]) {
  MNN_WAVE_SYNC();
  mnn_for<4>([&](auto s) MNN_INLINE { scr[j * 16 + 4 * s + q] = v[s]; });
  MNN_WAVE_SYNC();
  mnn_for<4>([&](auto s) MNN_INLINE { out[s] = scr[s * 64 + lane]; });
}

// out = a o b over the T tiles of a layer (zero behind them)
__device__ __forceinline__ void adj_mul(bwd_ctiles a, bwd_ctiles b, int T, bwd_tiles out) {
  mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE { out[o] = o < T ? a[o] * b[o] : bwd_zero(); });
}

// h = ELU(p) (VALUE) or D = ELU'(p) (!VALUE) of a layer; `h` is also the next layer's input
template <bool VALUE> __device__ __forceinline__ void adj_act(bwd_ctiles p, int T, bwd_tiles h, bwd_tiles D) {
  mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE {
    h[o] = bwd_zero();
    if constexpr (!VALUE) D[o] = bwd_zero();
    if (o < T) {
      mnn_for<4>([&](auto r) MNN_INLINE {
        if constexpr (VALUE) {
          h[o][(int)r] = mnn_elu(p[o][(int)r]);
        } else {
          float av, ad;
          mnn_elu(p[o][(int)r], av, ad);
          h[o][(int)r] = av;
          D[o][(int)r] = ad;
        }
      });
    }
  });
}

// The value forward of the wave's rows.  VALUE = false: D_l of every hidden layer and the field fo (register r: feature 4 r + q); VALUE = true: h_l of
// every hidden layer (the second evaluation of a stage, behind the feature loop).
template <int NH, bool VALUE>
__device__ __forceinline__ void adj_forward(const CnfLayout& L, const float* lds, const float* __restrict__ prow, int lane, int q, const float (&emb)[4], const float (&xin)[4],
                                            mnn_f4 (&H)[3][MNN_BWD_TM], mnn_f4 (&D)[3][MNN_BWD_TM], float (&fo)[4]) {
  constexpr int TM = MNN_BWD_TM;
  mnn_f4 p[TM], v[TM];
  mnn_for<TM>([&](auto o) MNN_INLINE {
    if (o < L.T[0]) p[o] = cnf_first_layer(L, lds, prow, lane, q, o, emb, xin);
  });
  if constexpr (VALUE) adj_act<true>(p, L.T[0], H[0], D[0]); else adj_act<false>(p, L.T[0], v, D[0]);
  if constexpr (NH > 1) {
    if constexpr (VALUE) adj_mv(lds + L.o_w[1], lds + L.o_b[1], L.T[0], L.T[1], lane, q, H[0], p); else adj_mv(lds + L.o_w[1], lds + L.o_b[1], L.T[0], L.T[1], lane, q, v, p);
    if constexpr (VALUE) adj_act<true>(p, L.T[1], H[1], D[1]); else adj_act<false>(p, L.T[1], v, D[1]);
  }
  if constexpr (NH > 2) {
    if constexpr (VALUE) adj_mv(lds + L.o_w[2], lds + L.o_b[2], L.T[1], L.T[2], lane, q, H[1], p); else adj_mv(lds + L.o_w[2], lds + L.o_b[2], L.T[1], L.T[2], lane, q, v, p);
    if constexpr (VALUE) adj_act<true>(p, L.T[2], H[2], D[2]); else adj_act<false>(p, L.T[2], v, D[2]);
  }
  if constexpr (!VALUE) {  // the last layer, as in cnf_field of csrc/cnf.hip: its rows are stored so that register r of lane (j, q) is feature 4 r + q
    const int tl = L.T[NH - 1];
    mnn_f4 c = *reinterpret_cast<const mnn_f4*>(lds + L.o_bo + q * 4);
    mnn_for<TM>([&](auto it) MNN_INLINE {
      if (it < tl) {
        const mnn_f4 a = *reinterpret_cast<const mnn_f4*>(lds + L.o_wo + it * 256 + lane * 4);
        mnn_for<4>([&](auto r) MNN_INLINE { c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[(int)r], v[it][(int)r], c, 0, 0, 0); });
      }
    });
    mnn_for<4>([&](auto r) MNN_INLINE { fo[r] = c[(int)r]; });
  }
}

// dst[unit] += scale times the sum over the wave's rows of v (lanes j = 0 own dst: nobody else reads or writes it)
__device__ __forceinline__ void adj_colsum(float* dst, bwd_ctiles v, float scale, int T, int j, int q) {
  mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE {
    if (o < T) {
      mnn_f4 s;
      mnn_for<4>([&](auto r) MNN_INLINE { s[(int)r] = bwd_sum_j(v[o][(int)r] * scale); });
      if (j == 0) {
        mnn_f4* d = reinterpret_cast<mnn_f4*>(dst + o * 16 + q * 4);
        *d = *d + s;
      }
    }
  });
}

// acc (feature j, units 16 o + 4 q + r) += the sum over the wave's rows of v, kept by the lanes j = i: a weight's column (or row) of feature i
__device__ __forceinline__ void adj_put_feature(bwd_tiles acc, bwd_ctiles v, int T, int j, int i) {
  mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE {
    if (o < T) {
      mnn_for<4>([&](auto r) MNN_INLINE {
        const float s = bwd_sum_j(v[o][(int)r]);
        acc[o][(int)r] += j == i ? s : 0.f;
      });
    }
  });
}

// The tangent of feature i forward and back: Db_l += Tb_l o Z_l, and the trace term's share of every weight gradient, scaled by sigma
template <int NH>
__device__ __forceinline__ void adj_tangent(const CnfLayout& L, const CnfAdjLayout& B, const float* lds, float* scr, int lane, int j, int q, int i, float beta, float sigma,
                                            const mnn_f4 (&D)[3][MNN_BWD_TM], mnn_f4 (&Db)[3][MNN_BWD_TM], mnn_f4 (&aW1)[MNN_BWD_TM][MNN_BWD_TM],
                                            mnn_f4 (&aW2)[MNN_BWD_TM][MNN_BWD_TM], bwd_tiles aWo, bwd_tiles aW0x) {
  constexpr int TM = MNN_BWD_TM;
  const int T0 = L.T[0], T1 = L.T[1], T2 = L.T[2], TL = L.T[NH - 1];
  const float* const w0c = lds + L.o_w0c + i * T0 * 16 + q * 4;
  const float* const wl = lds + L.o_wl + i * TL * 16 + q * 4;
  mnn_f4 Z2[TM], Z3[TM], Tt[TM], Tb[TM], Zb[TM];
  auto first = [&](bwd_tiles out) MNN_INLINE {  // T_1 = D_1 o W0x[:, i] (Z_1 = W0x[:, i] is read where it is used)
    mnn_for<TM>([&](auto o) MNN_INLINE { out[o] = o < T0 ? D[0][o] * *reinterpret_cast<const mnn_f4*>(w0c + o * 16) : bwd_zero(); });
  };
  first(Tt);
  if constexpr (NH > 1) adj_mv(lds + L.o_w[1], nullptr, T0, T1, lane, q, Tt, Z2);
  if constexpr (NH > 2) {
    adj_mul(D[1], Z2, T1, Tt);
    adj_mv(lds + L.o_w[2], nullptr, T1, T2, lane, q, Tt, Z3);
  }
  // the last layer: Tb_L = beta W_last[i, :], g W_last[i, :] += sigma beta T_L
  if constexpr (NH == 2) adj_mul(D[1], Z2, T1, Tt);
  if constexpr (NH == 3) adj_mul(D[2], Z3, T2, Tt);
  const float sb = sigma * beta;
  mnn_for<TM>([&](auto o) MNN_INLINE {
    Tb[o] = o < TL ? *reinterpret_cast<const mnn_f4*>(wl + o * 16) * beta : bwd_zero();
    Tt[o] = Tt[o] * sb;
  });
  adj_put_feature(aWo, Tt, TL, j, i);
  if constexpr (NH > 2) {
    mnn_for<TM>([&](auto o) MNN_INLINE {
      if (o < T2) Db[2][o] += Tb[o] * Z3[o];
    });
    adj_mul(Tb, D[2], T2, Zb);
    adj_mul(D[1], Z2, T1, Tt);
    bwd_outer<1, true>(scr, lane, j, q, T2, T1, &Zb, &Tt, aW2, sigma);
    adj_mv(lds + B.o_wT[2], nullptr, T2, T1, lane, q, Zb, Tb);
  }
  if constexpr (NH > 1) {
    mnn_for<TM>([&](auto o) MNN_INLINE {
      if (o < T1) Db[1][o] += Tb[o] * Z2[o];
    });
    adj_mul(Tb, D[1], T1, Zb);
    first(Tt);
    bwd_outer<1, true>(scr, lane, j, q, T1, T0, &Zb, &Tt, aW1, sigma);
    adj_mv(lds + B.o_wT[1], nullptr, T1, T0, lane, q, Zb, Tb);
  }
  mnn_for<TM>([&](auto o) MNN_INLINE {
    if (o < T0) Db[0][o] += Tb[o] * *reinterpret_cast<const mnn_f4*>(w0c + o * 16);
    Tt[o] = Tb[o] * D[0][o] * sigma;
  });
  adj_put_feature(aW0x, Tt, T0, j, i);
}

// Hutchinson's estimate eps^T (df/dx) eps in place of the trace: ONE tangent, in the row's direction ep (held as a state: features 4 s + q, zero
// behind F), forward and back.  Z_1 = W0x ep is a matrix product here (the x part of cnf_first_layer) and is formed again where Db_1 needs it,
// as adj_tangent reads its column again; the seed Tb_L = W_last^T (beta ep) is the product that forms hb from `as`; the two gradients that are a
// weight's column per feature in adj_tangent are outer products over the wave's rows here, those of the value reverse with ep for `as` and for x.
// There is no gradient for ep.
template <int NH>
__device__ __forceinline__ void adj_probe(const CnfLayout& L, const CnfAdjLayout& B, const float* lds, float* scr, int lane, int j, int q, const float (&ep)[4], float beta,
                                          float sigma, const mnn_f4 (&D)[3][MNN_BWD_TM], mnn_f4 (&Db)[3][MNN_BWD_TM], mnn_f4 (&aW1)[MNN_BWD_TM][MNN_BWD_TM],
                                          mnn_f4 (&aW2)[MNN_BWD_TM][MNN_BWD_TM], bwd_tiles aWo, bwd_tiles aW0x) {
  constexpr int TM = MNN_BWD_TM;
  const int T0 = L.T[0], T1 = L.T[1], T2 = L.T[2], TL = L.T[NH - 1];
  const float* const px = lds + L.o_w0x + lane;
  mnn_f4 Z2[TM], Z3[TM], Tt[TM], Tb[TM], Zb[TM];
  auto z1 = [&](auto o) MNN_INLINE {  // tile o of Z_1 = W0x ep
    mnn_f4 z = bwd_zero();
    mnn_for<4>([&](auto s) MNN_INLINE {
      if (s < L.kx) z = __builtin_amdgcn_mfma_f32_16x16x4f32(px[(o * L.kx + s) * 64], ep[s], z, 0, 0, 0);
    });
    return z;
  };
  auto first = [&](bwd_tiles out) MNN_INLINE {  // T_1 = D_1 o Z_1
    mnn_for<TM>([&](auto o) MNN_INLINE { out[o] = o < T0 ? D[0][o] * z1(o) : bwd_zero(); });
  };
  first(Tt);
  if constexpr (NH > 1) adj_mv(lds + L.o_w[1], nullptr, T0, T1, lane, q, Tt, Z2);
  if constexpr (NH > 2) {
    adj_mul(D[1], Z2, T1, Tt);
    adj_mv(lds + L.o_w[2], nullptr, T1, T2, lane, q, Tt, Z3);
  }
  // the last layer: Tb_L = W_last^T (beta ep), g W_last += sigma beta ep T_L^T
  if constexpr (NH == 2) adj_mul(D[1], Z2, T1, Tt);
  if constexpr (NH == 3) adj_mul(D[2], Z3, T2, Tt);
  float EB[4];
  adj_state_transpose(scr + 256, ep, lane, j, q, EB);
  {
    const float sb = sigma * beta;
    const float* const pw = lds + B.o_woT + lane;
    mnn_for<TM>([&](auto o) MNN_INLINE {
      Tb[o] = bwd_zero();
      if (o < TL) {
        mnn_for<4>([&](auto k) MNN_INLINE {
          if (k < L.kx) Tb[o] = __builtin_amdgcn_mfma_f32_16x16x4f32(pw[(o * L.kx + k) * 64], beta * ep[k], Tb[o], 0, 0, 0);
        });
        float PA[4];
        const mnn_f4 sc = Tt[o] * sb;
        bwd_transpose(scr, sc, lane, j, q, PA);
        mnn_for<4>([&](auto k) MNN_INLINE { aWo[o] = __builtin_amdgcn_mfma_f32_16x16x4f32(PA[k], EB[k], aWo[o], 0, 0, 0); });
      }
    });
  }
  if constexpr (NH > 2) {
    mnn_for<TM>([&](auto o) MNN_INLINE {
      if (o < T2) Db[2][o] += Tb[o] * Z3[o];
    });
    adj_mul(Tb, D[2], T2, Zb);
    adj_mul(D[1], Z2, T1, Tt);
    bwd_outer<1, true>(scr, lane, j, q, T2, T1, &Zb, &Tt, aW2, sigma);
    adj_mv(lds + B.o_wT[2], nullptr, T2, T1, lane, q, Zb, Tb);
  }
  if constexpr (NH > 1) {
    mnn_for<TM>([&](auto o) MNN_INLINE {
      if (o < T1) Db[1][o] += Tb[o] * Z2[o];
    });
    adj_mul(Tb, D[1], T1, Zb);
    first(Tt);
    bwd_outer<1, true>(scr, lane, j, q, T1, T0, &Zb, &Tt, aW1, sigma);
    adj_mv(lds + B.o_wT[1], nullptr, T1, T0, lane, q, Zb, Tb);
  }
  // the first layer: Db_1 += Tb_1 o Z_1, g W0x += sigma (Tb_1 o D_1) ep^T (ep transposed again: four registers less across the hidden layers)
  if constexpr (NH > 1) adj_state_transpose(scr + 256, ep, lane, j, q, EB);
  mnn_for<TM>([&](auto o) MNN_INLINE {
    if (o < T0) {
      Db[0][o] += Tb[o] * z1(o);
      float PA[4];
      const mnn_f4 sc = Tb[o] * D[0][o] * sigma;
      bwd_transpose(scr, sc, lane, j, q, PA);
      mnn_for<4>([&](auto k) MNN_INLINE { aW0x[o] = __builtin_amdgcn_mfma_f32_16x16x4f32(PA[k], EB[k], aW0x[o], 0, 0, 0); });
    }
  });
}

extern __shared__ __attribute__((aligned(16))) float cnf_adj_lds[];

// TAN: the trace term (al given); with PROBE (which implies TAN) Hutchinson's estimate along the row's eps instead of the exact trace
template <int NH, bool TAN, bool PROBE = false> __global__ __launch_bounds__(MNN_THREADS, 1) void cnf_adj_kernel(CnfAdjArgs a) {
  static_assert(TAN || !PROBE);
  constexpr int TM = MNN_BWD_TM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
  const CnfLayout& L = a.L;
  const CnfAdjLayout& B = a.B;
  float* const lds = cnf_adj_lds;
  float* const scr = cnf_adj_lds + a.lds_main + wave * MNN_BWD_SCRATCH;
  float* const cs = cnf_adj_lds + a.lds_main + (MNN_THREADS / 64) * MNN_BWD_SCRATCH + wave * CNF_ADJ_COLS;  // (touched by this wave's lanes j = 0 only)
  for (int i = lane; i < CNF_ADJ_COLS; i += 64) cs[i] = 0.f;
  mnn_stage_image(lds, a.image, B.total, tid);
  __syncthreads();

  const int T0 = L.T[0], T1 = L.T[1], T2 = L.T[2], TL = L.T[NH - 1];
  mnn_f4 aW1[TM][TM], aW2[TM][TM], aW0x[TM], aWo[TM];
  mnn_f4 aBo = bwd_zero();
  mnn_for<TM>([&](auto o) MNN_INLINE {
    mnn_for<TM>([&](auto i) MNN_INLINE { aW1[o][i] = bwd_zero(); aW2[o][i] = bwd_zero(); });
    aW0x[o] = aWo[o] = bwd_zero();
  });

  const float hstep = -a.dt;
  const long long r0 = (long long)blockIdx.x * a.rows_per_chunk;
  const long long r1 = r0 + a.rows_per_chunk < a.N ? r0 + a.rows_per_chunk : a.N;
  for (long long t0 = r0 + wave * 16; t0 < r1; t0 += (MNN_THREADS / 64) * 16) {
    const long long row = t0 + j;
    const bool valid = row < r1;
    const long long rc = valid ? row : a.N - 1;  // rows behind the end compute on the last row with zero adjoints and store nothing
    const float* const prow = a.pre + rc * a.ld_pre;
    float* const kb = a.kbuf + (t0 / 16) * CNF_ADJ_KTILE + lane;  // the wave's scratch: k vectors [stage][x | a][slot][lane], then the launch's g pre; a lane touches its own only
    // x and ax are read again where a sum starts from them: eight registers less across the feature loop
    auto state = [&](auto c, float& xv, float& avv) MNN_INLINE {
      const bool in = 4 * c + q < L.F;
      xv = in ? a.x[rc * a.ldx + 4 * c + q] : 0.f;
      avv = (in && valid) ? a.ax[row * a.ldax + 4 * c + q] : 0.f;
    };
    float beta = 0.f;
    if constexpr (TAN) beta = valid ? a.al[row] * a.tscale : 0.f;
#pragma unroll 1
    for (int s = 0; s < 6; ++s) {
      // the stage's inputs: x + A[s][0] k1 + A[s][1] k2 + ..., left to right (a zero entry adds nothing)
      float xs[4], as[4];
      mnn_for<4>([&](auto c) MNN_INLINE {
        float ux, ua;
        state(c, ux, ua);
        if (c < L.kx) {
          for (int m = 0; m < s; ++m) {
            ux = ux + CNF_A[s][m] * kb[((2 * m) * 4 + c) * 64];
            ua = ua + CNF_A[s][m] * kb[((2 * m + 1) * 4 + c) * 64];
          }
        }
        xs[c] = ux;
        as[c] = ua;
      });
      const float ts = a.t + CNF_C[s] * hstep;
      const float sigma = CNF_A[6][s] * a.dt;
      float emb[4];
      mnn_for<4>([&](auto k) MNN_INLINE {
        emb[k] = 0.f;
        if (k < L.kt) emb[k] = cnf_embed(L, lds, 4 * k + q, ts);
      });
      mnn_f4 H[3][TM], D[3][TM], Db[3][TM];
      float fo[4];
      adj_forward<NH, false>(L, lds, prow, lane, q, emb, xs, H, D, fo);
      mnn_for<4>([&](auto r) MNN_INLINE {
        if (r < L.kx) kb[((2 * s) * 4 + r) * 64] = hstep * fo[r];
      });
      mnn_for<3>([&](auto l) MNN_INLINE {
        mnn_for<TM>([&](auto o) MNN_INLINE { Db[l][o] = bwd_zero(); });
      });
      if constexpr (PROBE) {
        float ep[4];  // (read per stage, as x and ax are: nothing of it is held across the value passes)
        mnn_for<4>([&](auto c) MNN_INLINE { ep[c] = 4 * c + q < L.F ? a.eps[rc * a.ld_eps + 4 * c + q] : 0.f; });
        adj_probe<NH>(L, B, lds, scr, lane, j, q, ep, beta, sigma, D, Db, aW1, aW2, aWo, aW0x);
      } else if constexpr (TAN) {
#pragma unroll 1
        for (int i = 0; i < L.F; ++i) adj_tangent<NH>(L, B, lds, scr, lane, j, q, i, beta, sigma, D, Db, aW1, aW2, aWo, aW0x);
      }
      adj_forward<NH, true>(L, lds, prow, lane, q, emb, xs, H, D, fo);

      // ---- the value reverse
      mnn_f4 hb[TM], pb[TM];
      float AB[4];
      adj_state_transpose(scr + 256, as, lane, j, q, AB);
      {
        const float* const pw = lds + B.o_woT + lane;
        mnn_for<TM>([&](auto o) MNN_INLINE {
          hb[o] = bwd_zero();
          if (o < TL) {
            mnn_for<4>([&](auto k) MNN_INLINE {
              if (k < L.kx) hb[o] = __builtin_amdgcn_mfma_f32_16x16x4f32(pw[(o * L.kx + k) * 64], as[k], hb[o], 0, 0, 0);
            });
            float PA[4];
            const mnn_f4 sc = H[NH - 1][o] * sigma;
            bwd_transpose(scr, sc, lane, j, q, PA);
            mnn_for<4>([&](auto k) MNN_INLINE { aWo[o] = __builtin_amdgcn_mfma_f32_16x16x4f32(PA[k], AB[k], aWo[o], 0, 0, 0); });
          }
        });
        mnn_for<4>([&](auto c) MNN_INLINE { aBo[(int)c] += sigma * as[c]; });
      }
      auto local = [&](auto l, int T) MNN_INLINE {  // pb_l = D_l o hb_l + Db_l o D'_l
        mnn_for<TM>([&](auto o) MNN_INLINE {
          pb[o] = bwd_zero();
          if (o < T) {
            mnn_for<4>([&](auto r) MNN_INLINE {
              const float d1 = D[l][o][(int)r];
              float v = d1 * hb[o][(int)r];
              if constexpr (TAN) v += Db[l][o][(int)r] * (H[l][o][(int)r] > 0.f ? 0.f : d1);
              pb[o][(int)r] = v;
            });
          }
        });
      };
      if constexpr (NH > 2) {
        local(std::integral_constant<int, 2>{}, T2);
        adj_colsum(cs + 64, pb, sigma, T2, j, q);
        bwd_outer<1, true>(scr, lane, j, q, T2, T1, &pb, &H[1], aW2, sigma);
        adj_mv(lds + B.o_wT[2], nullptr, T2, T1, lane, q, pb, hb);
      }
      if constexpr (NH > 1) {
        local(std::integral_constant<int, 1>{}, T1);
        adj_colsum(cs, pb, sigma, T1, j, q);
        bwd_outer<1, true>(scr, lane, j, q, T1, T0, &pb, &H[0], aW1, sigma);
        adj_mv(lds + B.o_wT[1], nullptr, T1, T0, lane, q, pb, hb);
      }
      local(std::integral_constant<int, 0>{}, T0);
      // the first layer: g pre, g W0x += pb_1 x^T, g W0t += pb_1 emb^T, and W0x^T pb_1
      {
        float XB[4];
        adj_state_transpose(scr + 256, xs, lane, j, q, XB);
        adj_colsum(cs + 128 + s * 64, pb, sigma, T0, j, q);  // g W0t += pb_1 emb^T: emb is the same for every row, so the rows' sum is kept per stage
        mnn_f4 c = bwd_zero();
        mnn_for<TM>([&](auto o) MNN_INLINE {
          if (o < T0) {
            const mnn_f4 sc = pb[o] * sigma;
            {  // g pre of this launch: the stages' sum first (in the wave's scratch), added to gpre once behind the stages
              mnn_f4* const g = reinterpret_cast<mnn_f4*>(kb - lane + CNF_ADJ_KVECS + (o * 64 + lane) * 4);
              *g = s == 0 ? sc : *g + sc;
            }
            float PA[4];
            bwd_transpose(scr, sc, lane, j, q, PA);
            mnn_for<4>([&](auto k) MNN_INLINE {
              aW0x[o] = __builtin_amdgcn_mfma_f32_16x16x4f32(PA[k], XB[k], aW0x[o], 0, 0, 0);
            });
            const mnn_f4 w = *reinterpret_cast<const mnn_f4*>(lds + B.o_w0xT + o * 256 + lane * 4);
            mnn_for<4>([&](auto r) MNN_INLINE { c = __builtin_amdgcn_mfma_f32_16x16x4f32(w[(int)r], pb[o][(int)r], c, 0, 0, 0); });
          }
        });
        mnn_for<4>([&](auto r) MNN_INLINE {
          if (r < L.kx) kb[((2 * s + 1) * 4 + r) * 64] = a.dt * c[(int)r];
        });
      }
    }
    {
      mnn_for<4>([&](auto c) MNN_INLINE {
        float ux, ua;
        state(c, ux, ua);
        if (c < L.kx) {
          mnn_for<6>([&](auto m) MNN_INLINE { ua = ua + CNF_A[6][m] * kb[((2 * m + 1) * 4 + c) * 64]; });
        }
        if (valid && 4 * c + q < L.F) a.ax_next[row * a.ldan + 4 * c + q] = ua;
      });
      if (valid) {
        mnn_for<TM>([&](auto o) MNN_INLINE {
          if (o < T0) {
            mnn_f4* const g = reinterpret_cast<mnn_f4*>(a.gpre + row * a.ld_gpre + o * 16 + q * 4);
            *g = *g + *reinterpret_cast<const mnn_f4*>(kb - lane + CNF_ADJ_KVECS + (o * 64 + lane) * 4);
          }
        });
      }
    }
  }
  if (!a.work) return;  // (uniform over the grid: nobody asked for parameter gradients)

  float ej[6];  // emb(t_s)[j] of the six stages, for g W0t (read from the image before the partial overwrites it)
  mnn_for<6>([&](auto s) MNN_INLINE { ej[s] = cnf_embed(L, lds, j, a.t + CNF_C[s] * hstep); });

  // ---- the block's four waves, added in the order 0, 1, 2, 3 over the LDS the image occupied
  float* const G = lds;
  for (int w = 0; w < MNN_THREADS / 64; ++w) {
    __syncthreads();
    if (wave == w) {
      const bool set = w == 0;
      mnn_for<TM>([&](auto o) MNN_INLINE {
        if (o < T0) {
          mnn_f4 w0t = bwd_zero();
          mnn_for<6>([&](auto s) MNN_INLINE { w0t += *reinterpret_cast<const mnn_f4*>(cs + 128 + s * 64 + o * 16 + q * 4) * ej[s]; });
          mnn_f4* d0 = reinterpret_cast<mnn_f4*>(G + B.g_w0t + o * 256 + lane * 4);
          mnn_f4* d1 = reinterpret_cast<mnn_f4*>(G + B.g_w0x + o * 256 + lane * 4);
          *d0 = set ? w0t : *d0 + w0t;
          *d1 = set ? aW0x[o] : *d1 + aW0x[o];
        }
        if (o < TL) {
          mnn_f4* d = reinterpret_cast<mnn_f4*>(G + B.g_wo + o * 256 + lane * 4);
          *d = set ? aWo[o] : *d + aWo[o];
        }
      });
      if constexpr (NH > 1) {
        bwd_put_tiles<TM>(G + B.g_w[1], aW1, T1, T0, lane, set);
        if (lane < T1 * 16) G[B.g_b[1] + lane] = set ? cs[lane] : G[B.g_b[1] + lane] + cs[lane];
      }
      if constexpr (NH > 2) {
        bwd_put_tiles<TM>(G + B.g_w[2], aW2, T2, T1, lane, set);
        if (lane < T2 * 16) G[B.g_b[2] + lane] = set ? cs[64 + lane] : G[B.g_b[2] + lane] + cs[64 + lane];
      }
      mnn_f4 sb;
      mnn_for<4>([&](auto r) MNN_INLINE { sb[(int)r] = bwd_sum_j(aBo[(int)r]); });
      if (j == 0) {
        mnn_f4* d = reinterpret_cast<mnn_f4*>(G + B.g_bo + q * 4);
        *d = set ? sb : *d + sb;
      }
    }
  }
  __syncthreads();
  float* out = a.work + (size_t)blockIdx.x * B.g_total;
  for (int i = tid * 4; i < B.g_total; i += MNN_THREADS * 4) *reinterpret_cast<mnn_f4*>(out + i) = *reinterpret_cast<const mnn_f4*>(G + i);
}

// gparams[table[pos]] += the chunks' partials of pos added in chunk order (every parameter has one position: one writer)
__global__ __launch_bounds__(256) void cnf_adj_reduce_kernel(const float* __restrict__ work, const int* __restrict__ table, float* __restrict__ gparams, int chunks,
                                                             int g_total, long long flat_total) {
  const int pos = blockIdx.x * 256 + threadIdx.x;
  if (pos >= g_total) return;
  const long long dst = table[pos];
  if (dst < 0 || dst >= flat_total) return;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += work[(size_t)c * g_total + pos];
  gparams[dst] += s;
}

// the launcher of both argument blocks: P is zk_cnf_adj_args_v1 (eps = NULL) or zk_cnf_adj_args_v2, whose first fields are v1's
template <class P> static int cnf_adjoint_step(const P* p, uint32_t version, const void* eps, long long ld_eps, void* stream) {
  if (!p || p->struct_size != sizeof(P) || p->version != version) return ZK_EINVAL;
  CnfAdjArgs a;
  if (!cnf_adj_shape(p->features, p->freqs, p->n_hidden, p->width0, p->width1, p->width2, &a.L, &a.B)) return ZK_EINVAL;
  if (p->image_floats != a.B.total || p->grad_floats != a.B.g_total || p->N < 0) return ZK_EINVAL;
  if (p->ldx < p->features || p->ld_ax < p->features || p->ld_ax_next < p->features) return ZK_EINVAL;
  if (!cnf_step_fields_ok(p, true) || p->ld_gpre < p->width0 || p->ld_gpre % 4 != 0) return ZK_EINVAL;
  if (p->gparams && p->flat_total < 1) return ZK_EINVAL;
  if (!p->ax || !p->ax_next) return ZK_EINVAL;
  if (p->N == 0) return 0;
  if (!p->x || !p->pre || !p->image || !p->gpre || !p->work) return ZK_EINVAL;
  if (p->gparams && !p->grad_table) return ZK_EINVAL;
  if (eps && ld_eps < p->features) return ZK_EINVAL;
  if (!p->al) eps = nullptr;  // the estimator belongs to the trace term: without al the probe is not read
  if (((uintptr_t)p->pre | (uintptr_t)p->image | (uintptr_t)p->gpre | (uintptr_t)p->work) % 16 != 0) return ZK_EINVAL;
  int chunks = 0;
  if (mnn_bwd_geometry(p->N, 1, CNF_ADJ_BLOCKS, &a.rows_per_chunk, &chunks) != 0) return ZK_EINVAL;
  a.x = (const float*)p->x; a.ax = (const float*)p->ax; a.al = (const float*)p->al; a.pre = (const float*)p->pre; a.image = (const float*)p->image;
  a.eps = (const float*)eps; a.ld_eps = ld_eps;
  a.ax_next = (float*)p->ax_next; a.gpre = (float*)p->gpre; a.work = p->gparams ? (float*)p->work : nullptr;
  a.kbuf = (float*)p->work + (size_t)chunks * a.B.g_total;  // (behind the partials: the stages' k vectors, written and read by the lane that owns them)
  a.N = p->N; a.ldx = p->ldx; a.ldax = p->ld_ax; a.ldan = p->ld_ax_next; a.ld_pre = p->ld_pre; a.ld_gpre = p->ld_gpre;
  a.t = (float)p->t; a.dt = (float)p->dt; a.tscale = (float)p->trace_scale;
  a.lds_main = a.B.total > a.B.g_total ? a.B.total : a.B.g_total;
  const bool tan = p->al != nullptr;
  const void* fn = eps ? (a.L.nh == 1 ? (const void*)cnf_adj_kernel<1, true, true> : a.L.nh == 2 ? (const void*)cnf_adj_kernel<2, true, true> : (const void*)cnf_adj_kernel<3, true, true>)
                 : a.L.nh == 1 ? (tan ? (const void*)cnf_adj_kernel<1, true> : (const void*)cnf_adj_kernel<1, false>)
                 : a.L.nh == 2 ? (tan ? (const void*)cnf_adj_kernel<2, true> : (const void*)cnf_adj_kernel<2, false>)
                               : (tan ? (const void*)cnf_adj_kernel<3, true> : (const void*)cnf_adj_kernel<3, false>);
  hipStream_t st = (hipStream_t)stream;
  const int rc = mnn_launch_dyn_lds(fn, dim3((unsigned)chunks), cnf_adj_lds_floats(a.B) * 4, &a, st);
  if (rc != 0 || !a.work) return rc;
  hipLaunchKernelGGL(cnf_adj_reduce_kernel, dim3((unsigned)((a.B.g_total + 255) / 256)), dim3(256), 0, st, (const float*)a.work, (const int*)p->grad_table, (float*)p->gparams,
                     chunks, a.B.g_total, (long long)p->flat_total);
  return ZK_LAUNCH_CHECK();
}

}  // namespace zk

extern "C" int zk_cnf_adjoint_step(const zk_cnf_adj_args_v1* args, void* stream) { return zk::cnf_adjoint_step(args, 1, nullptr, 0, stream); }
extern "C" int zk_cnf_adjoint_step_v2(const zk_cnf_adj_args_v2* args, void* stream) {
  return zk::cnf_adjoint_step(args, 2, args ? args->eps : nullptr, args ? (long long)args->ld_eps : 0, stream);
}
extern "C" int zk_cnf_adjoint_floats(int features, int freqs, int n_hidden, int width0, int width1, int width2, int* image_floats, int* grad_floats) {
  zk::CnfLayout L;
  zk::CnfAdjLayout B;
  if (!image_floats || !grad_floats || !zk::cnf_adj_shape(features, freqs, n_hidden, width0, width1, width2, &L, &B)) return ZK_EINVAL;
  *image_floats = B.total;
  *grad_floats = B.g_total;
  return 0;
}
extern "C" int zk_cnf_adjoint_geometry(int64_t N, int* rows_per_chunk, int* n_chunks) { return zk::mnn_bwd_geometry(N, 1, CNF_ADJ_BLOCKS, rows_per_chunk, n_chunks); }
extern "C" int zk_cnf_adjoint_workspace_floats(int64_t N, int features, int freqs, int n_hidden, int width0, int width1, int width2, int64_t* floats) {
  zk::CnfLayout L;
  zk::CnfAdjLayout B;
  if (!floats || !zk::cnf_adj_shape(features, freqs, n_hidden, width0, width1, width2, &L, &B)) return ZK_EINVAL;
  *floats = 0;
  if (N == 0) return 0;
  int rows = 0, chunks = 0;
  if (zk::mnn_bwd_geometry(N, 1, CNF_ADJ_BLOCKS, &rows, &chunks) != 0) return ZK_EINVAL;
  *floats = (int64_t)chunks * B.g_total + ((N + 15) / 16) * CNF_ADJ_KTILE;
  return 0;
}
