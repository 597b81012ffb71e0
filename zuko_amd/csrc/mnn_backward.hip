// zuko_amd — adjoint of the monotone neural network of the neural autoregressive flow (NAF): the gradients of (y, ladj = log dy/dx) of
// csrc/mnn.hip with respect to x, the signal and every weight and bias of the per-feature networks.
//
// Per element (n, column j of feature f), with A_l = |W_l[f]|, u = (x, s_1..s_S), a0x = A_0[:, 0], the forward is
//     p_0 = A_0 u + b_0      pd_0 = a0x
//     p_l = A_l v_{l-1} + b_l    pd_l = A_l t_{l-1}        v_l = act(p_l)    t_l = act'(p_l) * pd_l
//     y = a_L . v_last + b_L     dy = a_L . t_last         ladj = log dy
// and the reverse sweep for upstream (gy, gl), k = gl / dy:
//     vb_last = gy a_L    tb_last = k a_L    g a_L += gy v_last + k t_last    g b_L += gy
//     pb_l = vb_l act'(p_l) + tb_l act''(p_l) pd_l      pdb_l = tb_l act'(p_l)      g b_l += pb_l
//     l >= 1:  g A_l += pb_l v_{l-1}^T + pdb_l t_{l-1}^T     vb_{l-1} = A_l^T pb_l     tb_{l-1} = A_l^T pdb_l
//     l = 0:   g A_0 += pb_0 u^T,  g A_0[:, 0] += pdb_0      gx = a0x . pb_0           gsignal = A_0[:, 1:]^T pb_0
//     g W_l = sign(W_l) g A_l
//
// Execution model (gfx950), the forward kernel's:
//   * a wavefront owns 16 elements of ONE feature; the forward is recomputed, p_l and pd_l stay in registers (nothing was saved by the forward
//     launch); lane (j, q) = (lane & 15, lane >> 4) holds units 16 o + 4 q + r of element j (the D fragment of v_mfma_f32_16x16x4_f32).
//   * one feature's BACKWARD image sits in LDS: the forward image followed by the same weights in transposed tile order (zuko_amd/mnn_plan.py:
//     layout_backward), so that A_l^T pb is the forward's product with the roles of `in` and `out` exchanged: one conflict-free 16-byte read per
//     lane and tile, pb in the D layout is the B operand as it stands.
//   * the weight gradients contract over the wave's 16 ELEMENTS: both operands are transposes of what the lanes hold.  A 16 x 16 fragment goes
//     through 256 floats of per-wave LDS as M[element][unit] (one 16-byte write per lane, rows of 16 floats), and k-step s of either operand is
//     M[64 s + lane]: consecutive addresses, no bank conflict.  Only the wave itself touches its scratch: s_waitcnt + wave_barrier, no
//     workgroup barrier inside the row loop.
//   * a block covers one column and one row chunk (zk_mnn_backward_geometry) and walks its row tiles with the gradient of every weight in
//     accumulator registers; bias-like gradients are per-lane sums, added over the 16 element lanes once, at the end.  The block's four waves
//     are then added in LDS in the order 0, 1, 2, 3 and ONE partial per (row chunk, column) is written.  No atomics.
//   * mnn_bwd_reduce_kernel adds the partials in chunk order, applies sign(W) and scatters through the gradient table (the inverse of the
//     partial's layout) into the flat parameter order; columns name distinct features, so every parameter has one writer.
// The layouts, the geometry, the transpose, the partial stores and the reduction's launch are shared with UNAF's adjoint (csrc/umnn_backward.hip)
// through csrc/zk_mnn_bwd_common.h; the reduction kernel itself lives here, with a flag for the family whose weights are signed.
#include "zk_mnn_bwd_common.h"

namespace zk {

struct MnnBwdArgs {
  const float* x;
  const float* signal;
  const float* image;
  const int* feat;
  const float* gy;
  const float* gl;
  float* gx;
  float* gsignal;
  float* work;
  long long N, ldx, lds, ldgx, ldgs;
  int Dsel, n_features, rows_per_chunk, gl_reduced, lds_main;
  MnnLayout L;
  MnnBwdLayout B;
};

// v = act(p), t = act'(p) * pd for the T tiles of a layer (the two-way ELU of csrc/mnn.hip)
__device__ __forceinline__ void bwd_act(bwd_ctiles p, bwd_ctiles pd, int T, int q, bwd_tiles v, bwd_tiles t) {
  const int half = (T * 16 + 1) / 2;
  mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE {
    if (o < T) {
      mnn_for<4>([&](auto r) MNN_INLINE {
        const bool first = o * 16 + q * 4 + r < half;
        const float pr = p[o][(int)r];
        float a, d;
        mnn_elu(first ? pr : -pr, a, d);
        v[o][(int)r] = first ? a : -a;
        t[o][(int)r] = d * pd[o][(int)r];
      });
    }
  });
}

// pb = vb act'(p) + tb act''(p) pd, pdb = tb act'(p) (the second derivative wants exp(s) itself: not mnn_elu)
__device__ __forceinline__ void bwd_local(bwd_ctiles p, bwd_ctiles pd, int T, int q, bwd_ctiles vb, bwd_ctiles tb, bwd_tiles pb, bwd_tiles pdb) {
  const int half = (T * 16 + 1) / 2;
  mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE {
    pb[o] = bwd_zero();
    pdb[o] = bwd_zero();
    if (o < T) {
      mnn_for<4>([&](auto r) MNN_INLINE {
        const bool first = o * 16 + q * 4 + r < half;
        const float pr = p[o][(int)r];
        const float s = first ? pr : -pr;
        const float e = expf(s);
        const float d1 = s > 0.f ? 1.f : e;
        const float d2 = s > 0.f ? 0.f : (first ? e : -e);
        pb[o][(int)r] = vb[o][(int)r] * d1 + tb[o][(int)r] * d2 * pd[o][(int)r];
        pdb[o][(int)r] = tb[o][(int)r] * d1;
      });
    }
  });
}

// acc[o][i] += pb[o] v[i]^T + pdb[o] t[i]^T, contracted over the wave's 16 elements.  Not bwd_outer<2> of the header: that one adds member by member,
// this one k-step by k-step (pb v, then pdb t), and the order of the additions into one accumulator decides the bits.
__device__ __forceinline__ void bwd_outer(float* scr, int lane, int j, int q, int tout, int tin, bwd_ctiles pb, bwd_ctiles pdb, bwd_ctiles v, bwd_ctiles t,
                                          mnn_f4 (&acc)[MNN_BWD_TM][MNN_BWD_TM]) {
  float PA[MNN_BWD_TM][4], PT[MNN_BWD_TM][4];
  mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE {
    if (o < tout) {
      bwd_transpose(scr, pb[o], lane, j, q, PA[o]);
      bwd_transpose(scr + 256, pdb[o], lane, j, q, PT[o]);
    }
  });
  mnn_for<MNN_BWD_TM>([&](auto i) MNN_INLINE {
    if (i < tin) {
      float VB[4], TB[4];
      bwd_transpose(scr, v[i], lane, j, q, VB);
      bwd_transpose(scr + 256, t[i], lane, j, q, TB);
      mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE {
        if (o < tout) {
          mnn_for<4>([&](auto s) MNN_INLINE {
            acc[o][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(PA[o][s], VB[s], acc[o][i], 0, 0, 0);
            acc[o][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(PT[o][s], TB[s], acc[o][i], 0, 0, 0);
          });
        }
      });
    }
  });
}

extern __shared__ __attribute__((aligned(16))) float mnn_bwd_lds[];

template <int NH, int TS> __global__ __launch_bounds__(MNN_THREADS, 1) void mnn_bwd_kernel(MnnBwdArgs a) {
  constexpr int TM = MNN_BWD_TM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
  const MnnLayout& L = a.L;
  const MnnBwdLayout& B = a.B;
  const int col = blockIdx.y;
  int f = a.feat ? a.feat[col] : col;
  f = f < 0 ? 0 : (f >= a.n_features ? a.n_features - 1 : f);  // (a memory guard only: the caller checks the range)
  const float* img = a.image + (size_t)f * B.total;
  float* const lds = mnn_bwd_lds;
  float* const scr = mnn_bwd_lds + a.lds_main + wave * MNN_BWD_SCRATCH;
  mnn_stage_image(lds, img, B.total, tid);
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

    // ---- the forward, keeping the pre-activations p_l and their tangents pd_l
    mnn_f4 p0[TM], w0x[TM], P1[2][TM], P2[2][TM], VT[2][TM];  // the pairs (p_l, pd_l) and (v, t) go through a layer product together
    bwd_tiles p1 = P1[0], pd1 = P1[1], p2 = P2[0], pd2 = P2[1], v = VT[0], t = VT[1];
    mnn_signal<TM>(L, lds, a.signal + rc * a.lds + (size_t)col * L.S, lane, q, p0);
    mnn_for<TM>([&](auto o) MNN_INLINE {
      p1[o] = p2[o] = pd1[o] = pd2[o] = bwd_zero();
      if (o < T0) {
        w0x[o] = *reinterpret_cast<const mnn_f4*>(lds + L.o_w0x + o * 16 + q * 4);
        mnn_for<4>([&](auto r) MNN_INLINE { p0[o][(int)r] = fmaf(w0x[o][(int)r], xin, p0[o][(int)r]); });
      } else {
        p0[o] = w0x[o] = bwd_zero();
      }
    });
    bwd_act(p0, w0x, T0, q, v, t);
    if constexpr (NH > 1) {
      bwd_mv<2, 1>(lds + L.o_w[1], lds + L.o_b[1], T0, T1, lane, q, VT, P1);
      bwd_act(p1, pd1, T1, q, v, t);
    }
    if constexpr (NH > 2) {
      bwd_mv<2, 1>(lds + L.o_w[2], lds + L.o_b[2], T1, T2, lane, q, VT, P2);
      bwd_act(p2, pd2, T2, q, v, t);
    }

    // ---- the last layer
    mnn_f4 VB[2][TM], PB[2][TM];  // (vb, tb) and (pb, pdb)
    bwd_tiles vb = VB[0], tb = VB[1], pb = PB[0], pdb = PB[1];
    {
      mnn_f4 wl[TM];
      float pdy = 0.f;
      mnn_for<TM>([&](auto o) MNN_INLINE {
        wl[o] = bwd_zero();
        if (o < TL) {
          wl[o] = *reinterpret_cast<const mnn_f4*>(lds + L.o_wl + o * 16 + q * 4);
          mnn_for<4>([&](auto r) MNN_INLINE { pdy = fmaf(wl[o][(int)r], t[o][(int)r], pdy); });
        }
      });
      const float dy = mnn_sum_q(pdy);
      const float k = glv / dy;
      mnn_for<TM>([&](auto o) MNN_INLINE {
        vb[o] = tb[o] = bwd_zero();
        if (o < TL) {
          mnn_for<4>([&](auto r) MNN_INLINE {
            vb[o][(int)r] = gyv * wl[o][(int)r];
            tb[o][(int)r] = k * wl[o][(int)r];
            aWl[o][(int)r] += gyv * v[o][(int)r] + k * t[o][(int)r];
          });
        }
      });
      if (q == 0) aBl += gyv;
    }

    // ---- the reverse sweep
    if constexpr (NH > 2) {
      bwd_local(p2, pd2, T2, q, vb, tb, pb, pdb);
      bwd_add(aB2, pb, T2);
      bwd_act(p1, pd1, T1, q, v, t);
      bwd_outer(scr, lane, j, q, T2, T1, pb, pdb, v, t, aW2);
      bwd_mv<2, 0>(lds + B.o_wT[2], nullptr, T2, T1, lane, q, PB, VB);  // (vb, tb) = A_2^T (pb, pdb)
    }
    if constexpr (NH > 1) {
      bwd_local(p1, pd1, T1, q, vb, tb, pb, pdb);
      bwd_add(aB1, pb, T1);
      bwd_act(p0, w0x, T0, q, v, t);
      bwd_outer(scr, lane, j, q, T1, T0, pb, pdb, v, t, aW1);
      bwd_mv<2, 0>(lds + B.o_wT[1], nullptr, T1, T0, lane, q, PB, VB);
    }
    bwd_local(p0, w0x, T0, q, vb, tb, pb, pdb);
    bwd_add(aB0, pb, T0);
    {
      float sx = 0.f;
      mnn_for<TM>([&](auto o) MNN_INLINE {
        if (o < T0) {
          mnn_for<4>([&](auto r) MNN_INLINE {
            aX[o][(int)r] += pb[o][(int)r] * xin + pdb[o][(int)r];
            sx = fmaf(w0x[o][(int)r], pb[o][(int)r], sx);
          });
        }
      });
      sx = mnn_sum_q(sx);
      if (a.gx && q == 0 && valid) a.gx[row * a.ldgx + col] = sx;
    }
    if (a.work) {  // g A_0[:, 1:] += pb_0 signal^T: the signal of element 4 s + q, feature 16 i + j, read in the operand's own layout
      float PA[TM][4];
      mnn_for<TM>([&](auto o) MNN_INLINE {
        if (o < T0) bwd_transpose(scr, pb[o], lane, j, q, PA[o]);
      });
      mnn_for<TS>([&](auto i) MNN_INLINE {
        if (i < B.ts) {
          const int sidx = i * 16 + j;
          mnn_for<4>([&](auto s) MNN_INLINE {
            const long long er = t0 + s * 4 + q;
            const long long ec = er < a.N ? er : a.N - 1;
            const float b = sidx < L.S ? a.signal[ec * a.lds + (size_t)col * L.S + sidx] : 0.f;
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
              mnn_for<4>([&](auto r) MNN_INLINE { gs = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[(int)r], pb[o][(int)r], gs, 0, 0, 0); });
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

// gparams[table[f][pos]] = the partials of (column, pos) added in chunk order, times sign(W) with `apply_sign` (NAF; UNAF's weights are signed)
__global__ __launch_bounds__(256) void mnn_bwd_reduce_kernel(const float* __restrict__ work, const int* __restrict__ table, const int* __restrict__ feat,
                                                             const float* __restrict__ params, float* __restrict__ gparams, int chunks, int Dsel, int g_total,
                                                             int n_features, long long flat_weights, long long flat_total, int apply_sign) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Dsel * g_total) return;
  const int col = (int)(idx / g_total), pos = (int)(idx % g_total);
  int f = feat ? feat[col] : col;
  if (f < 0 || f >= n_features) return;
  const long long dst = table[(size_t)f * g_total + pos];
  if (dst < 0 || dst >= flat_total) return;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += work[((size_t)c * Dsel + col) * g_total + pos];
  if (apply_sign && dst < flat_weights) {
    const float w = params[dst];
    s = w > 0.f ? s : (w < 0.f ? -s : 0.f);
  }
  gparams[dst] = s;
}

int mnn_bwd_reduce(const float* work, const int* table, const int* feat, const float* params, float* gparams, int chunks, int Dsel, int g_total, int n_features,
                   long long flat_weights, long long flat_total, bool apply_sign, hipStream_t st) {
  const long long n = (long long)Dsel * g_total;
  hipLaunchKernelGGL(mnn_bwd_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, work, table, feat, params, gparams, chunks, Dsel, g_total, n_features,
                     flat_weights, flat_total, apply_sign ? 1 : 0);
  return ZK_LAUNCH_CHECK();
}

template <int NH> static const void* mnn_bwd_fn(int ts) {
  if (ts <= 1) return (const void*)mnn_bwd_kernel<NH, 1>;
  if (ts <= 2) return (const void*)mnn_bwd_kernel<NH, 2>;
  return (const void*)mnn_bwd_kernel<NH, 4>;
}

static int mnn_backward(const zk_mnn_bwd_args_v1* p, void* stream) {
  if (!p || p->struct_size != sizeof(zk_mnn_bwd_args_v1) || p->version != 1) return ZK_EINVAL;
  MnnBwdArgs a;
  if (!mnn_bwd_shape(p->S, p->n_hidden, p->width0, p->width1, p->width2, &a.L, &a.B)) return ZK_EINVAL;
  if (p->image_floats != a.B.total || p->grad_floats != a.B.g_total || p->n_features < 1 || p->N < 0 || p->Dsel < 1 || p->Dsel > 65535) return ZK_EINVAL;
  if (p->ldx < 1 || p->ld_signal < p->Dsel * (int64_t)p->S) return ZK_EINVAL;
  if (p->gx && p->ld_gx < p->Dsel) return ZK_EINVAL;
  if (p->gsignal && p->ld_gsignal < p->Dsel * (int64_t)p->S) return ZK_EINVAL;
  if (p->gparams && (p->flat_total < 1 || p->flat_weights < 0 || p->flat_weights > p->flat_total)) return ZK_EINVAL;
  if (p->gparams && p->N > 0 && (!p->params || !p->grad_table || !p->work)) return ZK_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (p->N == 0) {
    if (p->gparams && hipMemsetAsync(p->gparams, 0, (size_t)p->flat_total * 4, st) != hipSuccess) return ZK_LAUNCH_CHECK();
    return 0;
  }
  if (!p->x || !p->signal || !p->image) return ZK_EINVAL;
  int chunks = 0;
  if (mnn_bwd_geometry(p->N, p->Dsel, MNN_BWD_BLOCKS, &a.rows_per_chunk, &chunks) != 0) return ZK_EINVAL;
  a.x = (const float*)p->x; a.signal = (const float*)p->signal; a.image = (const float*)p->image; a.feat = (const int*)p->feat;
  a.gy = (const float*)p->gy; a.gl = (const float*)p->gl; a.gx = (float*)p->gx; a.gsignal = (float*)p->gsignal;
  a.work = p->gparams ? (float*)p->work : nullptr;
  a.N = p->N; a.ldx = p->ldx; a.lds = p->ld_signal; a.ldgx = p->ld_gx; a.ldgs = p->ld_gsignal;
  a.Dsel = (int)p->Dsel; a.n_features = p->n_features; a.gl_reduced = p->gl_reduced;
  a.lds_main = a.B.total > a.B.g_total ? a.B.total : a.B.g_total;
  if (p->gparams && hipMemsetAsync(p->gparams, 0, (size_t)p->flat_total * 4, st) != hipSuccess) return ZK_LAUNCH_CHECK();
  if (!a.gx && !a.gsignal && !a.work) return 0;
  const void* fn = a.L.nh == 1 ? mnn_bwd_fn<1>(a.B.ts) : (a.L.nh == 2 ? mnn_bwd_fn<2>(a.B.ts) : mnn_bwd_fn<3>(a.B.ts));
  const int rc = mnn_launch_dyn_lds(fn, dim3((unsigned)chunks, (unsigned)a.Dsel), mnn_bwd_lds_floats(a.B) * 4, &a, st);
  if (rc != 0 || !a.work) return rc;
  return mnn_bwd_reduce((const float*)a.work, (const int*)p->grad_table, a.feat, (const float*)p->params, (float*)p->gparams, chunks, a.Dsel, a.B.g_total, a.n_features,
                        (long long)p->flat_weights, (long long)p->flat_total, true, st);
}

}  // namespace zk

extern "C" int zk_mnn_backward(const zk_mnn_bwd_args_v1* args, void* stream) { return zk::mnn_backward(args, stream); }
extern "C" int zk_mnn_backward_geometry(int64_t N, int64_t Dsel, int* rows_per_chunk, int* n_chunks) {
  return zk::mnn_bwd_geometry(N, Dsel, MNN_BWD_BLOCKS, rows_per_chunk, n_chunks);
}
extern "C" int zk_mnn_backward_floats(int S, int n_hidden, int width0, int width1, int width2, int* image_floats, int* grad_floats) {
  return zk::mnn_bwd_floats<0>(S, n_hidden, width0, width1, width2, image_floats, grad_floats);
}
extern "C" int zk_mnn_backward_workspace_floats(int64_t N, int64_t Dsel, int S, int n_hidden, int width0, int width1, int width2, int64_t* floats) {
  return zk::mnn_bwd_workspace_floats<0>(N, Dsel, S, n_hidden, width0, width1, width2, floats);
}
