// zuko_amd — what the adjoint kernels of the monotone networks of NAF (csrc/mnn_backward.hip) and UNAF (csrc/umnn_backward.hip) share: the layout
// of the backward image and of a gradient partial, the transpose of an accumulator fragment through per-wave LDS, the sums and stores that turn a
// wave's accumulators into the block's partial, the chunk reduction's launch and the host side of their size queries.  The reverse sweeps themselves
// (tangent chains for NAF, the quadrature's points for UNAF) and the two __global__ bodies are each family's own.
// With the adjoint of the continuous flow (csrc/cnf_backward.hip) as the third user: the chunk geometry (mnn_bwd_geometry, the block target a
// parameter) and the outer product over the wave's rows (bwd_outer<NP>; NAF's two-term one adds in another order and stays in its file).  The grouped
// layer product bwd_mv serves NAF and UNAF, forward and transposed; CNF keeps adj_mv, the three kernels keep their block tails and CNF its reduction
// kernel written out: profiles/small_net_frame/census.md says what each would have cost.
#pragma once
#include "zk_mnn_common.h"

namespace zk {

#define MNN_BWD_TM 4          // tiles per layer: widths <= 64
#define MNN_BWD_SCRATCH 512   // floats of transpose scratch per wavefront
#define MNN_BWD_BLOCKS 512    // the grid of the monotone networks' adjoints aims at this many blocks: two per CU
#define MNN_WAVE_SYNC() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); } while (0)

// Offsets (floats) behind the forward image, and of one (row chunk, column) partial; the arithmetic of zuko_amd/mnn_plan.py: layout_backward.
struct MnnBwdLayout {
  int ts;       // 16-wide tiles of the signal = ceil(S / 16)
  int o_wT[3];  // l = 1, 2: [T_{l-1}][T_l][256], lane (j, q), r of tile (i, o): |W_l[16 o + 4 q + r][16 i + j]|
  int o_w0sT;   // [ts][T_0][256], tile (i, o): |W_0[16 o + 4 q + r][1 + 16 i + j]| (zero behind S)
  int total;    // the backward image
  int g_w0s, g_w0x, g_b0, g_w[3], g_b[3], g_wl, g_bl, g_total;
};

static inline bool mnn_bwd_layout(const MnnLayout& L, MnnBwdLayout* B) {
  for (int l = 0; l < L.nh; ++l)
    if (L.T[l] > MNN_BWD_TM) return false;
  B->ts = (L.S + 15) / 16;
  int o = L.total;
  B->o_wT[0] = 0;
  for (int l = 1; l < 3; ++l) {
    B->o_wT[l] = o;
    if (l < L.nh) o += L.T[l] * L.T[l - 1] * 256;
  }
  B->o_w0sT = o; o += B->ts * L.T[0] * 256;
  B->total = o;
  int g = 0;
  B->g_w0s = g; g += L.T[0] * B->ts * 256;
  B->g_w0x = g; g += L.T[0] * 16;
  B->g_b0 = g; g += L.T[0] * 16;
  B->g_w[0] = B->g_b[0] = 0;
  for (int l = 1; l < 3; ++l) {
    B->g_w[l] = g; if (l < L.nh) g += L.T[l] * L.T[l - 1] * 256;
    B->g_b[l] = g; if (l < L.nh) g += L.T[l] * 16;
  }
  B->g_wl = g; g += L.T[L.nh - 1] * 16;
  B->g_bl = g; g += 4;
  B->g_total = g;
  return true;
}

static inline int mnn_bwd_lds_floats(const MnnBwdLayout& B) { return (B.total > B.g_total ? B.total : B.g_total) + (MNN_THREADS / 64) * MNN_BWD_SCRATCH; }

// rows per chunk (a multiple of 64) and the number of chunks of a grid that aims at `blocks` blocks: a pure function of the three sizes
static inline int mnn_bwd_geometry(long long N, long long Dsel, int blocks, int* rows_per_chunk, int* n_chunks) {
  if (N < 1 || Dsel < 1 || Dsel > 65535 || N > (1LL << 40) || !rows_per_chunk || !n_chunks) return ZK_EINVAL;
  long long want = blocks / Dsel;
  if (want < 1) want = 1;
  const long long t64 = (N + 63) / 64;
  if (want > t64) want = t64;
  const long long rows = ((t64 + want - 1) / want) * 64;
  if (rows > 0x7fffffc0LL) return ZK_EINVAL;
  *rows_per_chunk = (int)rows;
  *n_chunks = (int)((N + rows - 1) / rows);
  return 0;
}

// the layouts of a shape the adjoint kernels serve; `extra_lds_floats`: what a family keeps in LDS behind the transpose scratch
static inline bool mnn_bwd_shape(int S, int nh, int w0, int w1, int w2, MnnLayout* L, MnnBwdLayout* B, int extra_lds_floats = 0) {
  const int widths[3] = {w0, w1, w2};
  if (!mnn_layout(S, nh, widths, L)) return false;
  if (!mnn_bwd_layout(*L, B)) return false;
  return (mnn_bwd_lds_floats(*B) + extra_lds_floats) * 4 <= MNN_LDS_MAX;
}

// the image and gradient sizes of a shape, behind zk_mnn_backward_floats / zk_umnn_backward_floats (EXTRA: the family's extra_lds_floats)
template <int EXTRA> static inline int mnn_bwd_floats(int S, int nh, int w0, int w1, int w2, int* image_floats, int* grad_floats) {
  MnnLayout L;
  MnnBwdLayout B;
  if (!image_floats || !grad_floats || !mnn_bwd_shape(S, nh, w0, w1, w2, &L, &B, EXTRA)) return ZK_EINVAL;
  *image_floats = B.total;
  *grad_floats = B.g_total;
  return 0;
}

// one partial per (row chunk, column), behind zk_mnn_backward_workspace_floats / zk_umnn_backward_workspace_floats
template <int EXTRA> static inline int mnn_bwd_workspace_floats(long long N, long long Dsel, int S, int nh, int w0, int w1, int w2, int64_t* floats) {
  MnnLayout L;
  MnnBwdLayout B;
  if (!floats || !mnn_bwd_shape(S, nh, w0, w1, w2, &L, &B, EXTRA)) return ZK_EINVAL;
  *floats = 0;
  if (N == 0 && Dsel >= 1 && Dsel <= 65535) return 0;
  int rows = 0, chunks = 0;
  if (mnn_bwd_geometry(N, Dsel, MNN_BWD_BLOCKS, &rows, &chunks) != 0) return ZK_EINVAL;
  *floats = (int64_t)chunks * Dsel * B.g_total;
  return 0;
}

// gparams[table[f][pos]] = the partials of (column, pos) added in chunk order, times sign(W) for the weights when `apply_sign` (NAF: the image
// holds |W|; `params` are the signed flat parameters); on `st` (csrc/mnn_backward.hip holds the library's one kernel for it)
int mnn_bwd_reduce(const float* work, const int* table, const int* feat, const float* params, float* gparams, int chunks, int Dsel, int g_total, int n_features,
                   long long flat_weights, long long flat_total, bool apply_sign, hipStream_t st);

typedef mnn_f4 (&bwd_tiles)[MNN_BWD_TM];
typedef const mnn_f4 (&bwd_ctiles)[MNN_BWD_TM];

__device__ __forceinline__ mnn_f4 bwd_zero() { return mnn_f4{0.f, 0.f, 0.f, 0.f}; }

// A 16 x 16 fragment held as (element = j, units 4 q + r) becomes the four k-steps of a matrix operand that contracts over the elements:
// out[s] = fragment[unit = lane & 15][element = 4 s + (lane >> 4)].
__device__ __forceinline__ void bwd_transpose(float* scr, const mnn_f4& a, int lane, int j, int q, float (&out)[4]) {
  MNN_WAVE_SYNC();  // the reads of the fragment before this one are done
  *reinterpret_cast<mnn_f4*>(scr + j * 16 + q * 4) = a;
  MNN_WAVE_SYNC();
  mnn_for<4>([&](auto s) MNN_INLINE { out[s] = scr[s * 64 + lane]; });
}

// out[g] = W in[g] (+ b for the first NB members) for G right-hand sides at once, one out tile at a time: tiles [tout][tin][256] of the image, tile
// (o, it) at (o * tin + it) * 256.  It is the forward product of a layer on its forward tiles, and W^T's on the transposed tiles with the roles of
// `in` and `out` exchanged.  Every out tile is written (zero behind tout).  Per accumulator the matrix instructions go in the order (in tile, r); one
// read of a weight fragment feeds the G chains, g innermost.  in[g] / out[g] are the tile arrays of member g, as for mnn_matvec.
template <int G, int NB, class In, class Out>
__device__ __forceinline__ void bwd_mv(const float* W, const float* Bias, int tin, int tout, int lane, int q, In in, Out out) {
  mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE {
    mnn_for<G>([&](auto g) MNN_INLINE { out[g][o] = bwd_zero(); });
    if (o < tout) {
      if constexpr (NB > 0) {
        const mnn_f4 b = *reinterpret_cast<const mnn_f4*>(Bias + o * 16 + q * 4);
        mnn_for<NB>([&](auto g) MNN_INLINE { out[g][o] = b; });
      }
      mnn_for<MNN_BWD_TM>([&](auto it) MNN_INLINE {
        if (it < tin) {
          const mnn_f4 a0 = *reinterpret_cast<const mnn_f4*>(W + (o * tin + it) * 256 + lane * 4);
          mnn_for<4>([&](auto r) MNN_INLINE {
            mnn_for<G>([&](auto g) MNN_INLINE { out[g][o] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[(int)r], in[g][it][(int)r], out[g][o], 0, 0, 0); });
          });
        }
      });
    }
  });
}

// acc[o][i] += sum over the NP members, in order, of (scale pb[n][o]) v[n][i]^T, contracted over the wave's 16 rows; the scale exists with SCALED only
template <int NP, bool SCALED = false, class Pb, class V>
__device__ __forceinline__ void bwd_outer(float* scr, int lane, int j, int q, int tout, int tin, Pb pb, V v, mnn_f4 (&acc)[MNN_BWD_TM][MNN_BWD_TM], float scale = 1.f) {
  float PA[NP][MNN_BWD_TM][4];
  mnn_for<NP>([&](auto n) MNN_INLINE {
    mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE {
      if (o < tout) {
        if constexpr (SCALED) {
          const mnn_f4 sc = pb[n][o] * scale;
          bwd_transpose(scr, sc, lane, j, q, PA[n][o]);
        } else {
          bwd_transpose(scr, pb[n][o], lane, j, q, PA[n][o]);
        }
      }
    });
  });
  mnn_for<MNN_BWD_TM>([&](auto i) MNN_INLINE {
    if (i < tin) {
      float VB[NP][4];
      mnn_for<NP>([&](auto n) MNN_INLINE { bwd_transpose(scr + 256, v[n][i], lane, j, q, VB[n]); });
      mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE {
        if (o < tout) {
          mnn_for<NP>([&](auto n) MNN_INLINE {
            mnn_for<4>([&](auto s) MNN_INLINE { acc[o][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(PA[n][o][s], VB[n][s], acc[o][i], 0, 0, 0); });
          });
        }
      });
    }
  });
}

__device__ __forceinline__ void bwd_add(bwd_tiles acc, bwd_ctiles v, int T) {
  mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE {
    if (o < T) acc[o] += v[o];
  });
}

// sum over the 16 lanes that share q: the same value in all of them, the same order everywhere
__device__ __forceinline__ float bwd_sum_j(float p) {
  p += __shfl_xor(p, 1, 64);
  p += __shfl_xor(p, 2, 64);
  p += __shfl_xor(p, 4, 64);
  p += __shfl_xor(p, 8, 64);
  return p;
}

// the wave's share of a bias-like gradient (per-lane sums over the rows of element lane j) into the block's partial
__device__ __forceinline__ void bwd_put_units(float* G, bwd_ctiles acc, int T, int j, int q, bool set) {
  mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE {
    if (o < T) {
      mnn_f4 s;
      mnn_for<4>([&](auto r) MNN_INLINE { s[(int)r] = bwd_sum_j(acc[o][(int)r]); });
      if (j == 0) {
        mnn_f4* dst = reinterpret_cast<mnn_f4*>(G + o * 16 + q * 4);
        *dst = set ? s : *dst + s;
      }
    }
  });
}

template <int TI> __device__ __forceinline__ void bwd_put_tiles(float* G, const mnn_f4 (&acc)[MNN_BWD_TM][TI], int tout, int tin, int lane, bool set) {
  mnn_for<MNN_BWD_TM>([&](auto o) MNN_INLINE {
    mnn_for<TI>([&](auto i) MNN_INLINE {
      if (o < tout && i < tin) {
        mnn_f4* dst = reinterpret_cast<mnn_f4*>(G + (o * tin + i) * 256 + lane * 4);
        *dst = set ? acc[o][i] : *dst + acc[o][i];
      }
    });
  });
}

// the wave's share of a scalar gradient (per-lane sums over the rows) into the first of the four floats at G
__device__ __forceinline__ void bwd_put_scalar(float* G, float acc, int lane, bool set) {
  const float sb = bwd_sum_j(acc);
  if (lane == 0) {
    if (set) {
      G[0] = sb; G[1] = 0.f; G[2] = 0.f; G[3] = 0.f;
    } else {
      G[0] += sb;
    }
  }
}

}  // namespace zk
