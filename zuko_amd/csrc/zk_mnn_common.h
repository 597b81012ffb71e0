// zuko_amd — what the monotone-network kernels of NAF (csrc/mnn.hip) and UNAF (csrc/umnn.hip) share: the weight image's layout, the signal's share of
// the first layer, the four-lane sum, the launch geometry, the checks on the fields their two argument blocks have in common, and the launch with
// dynamic LDS.  The networks themselves (tangent, quadrature) and the two __global__ bodies are each family's own.
// For all six small-network kernels, the continuous flow's (csrc/cnf.hip) and the three adjoints included: ELU and its derivative (mnn_elu), the copy
// of an image into LDS (mnn_stage_image) and the paired layer product of the forward kernels that run two wavefronts per SIMD (mnn_matvec: mnn_hidden
// of NAF, the value and tangent products of CNF; umnn_hidden keeps its own unpaired one).  Where a kernel keeps a piece written out because the
// shared one moved its instruction census: profiles/small_net_frame/census.md.
#pragma once
#include "../../include/zuko_amd.h"
#include "zk_common.h"
#include <utility>

namespace zk {

typedef float mnn_f4 __attribute__((ext_vector_type(4)));

#define MNN_INLINE __attribute__((always_inline))
#define MNN_LDS_MAX (128 * 1024)  // bound on one feature's image (two blocks of the default network's 21 KiB share a CU many times over)
#define MNN_THREADS 256

template <class F, int... I> __device__ __forceinline__ void mnn_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F> __device__ __forceinline__ void mnn_for(F&& f) { mnn_for_impl(f, std::make_integer_sequence<int, N>{}); }

// Offsets (floats) of one feature's image; the same arithmetic as zuko_amd/mnn_plan.py: layout.
struct MnnLayout {
  int nh, S, ks;  // hidden layers, signal features, k-steps of the signal product = ceil(S / 4)
  int T[3];       // 16-unit tiles per hidden layer
  int o_w0s, o_w0x, o_b0, o_w[3], o_b[3], o_wl, o_bl, total;
};

static inline bool mnn_layout(int S, int nh, const int* widths, MnnLayout* L) {
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
  return o * 4 <= MNN_LDS_MAX;
}

// c0 = W0[:, 1:] signal + b0 in the D layout (T1 tiles), W0 as the image holds it: |W0| for NAF, signed for UNAF
template <int TM> __device__ __forceinline__ void mnn_signal(const MnnLayout& L, const float* lds, const float* __restrict__ sp, int lane, int q, mnn_f4 (&c0)[TM]) {
  float sig[16];
  mnn_for<16>([&](auto s) MNN_INLINE {
    sig[s] = 0.f;
    if (s < L.ks) sig[s] = (4 * s + q < L.S) ? sp[4 * s + q] : 0.f;
  });
  mnn_for<TM>([&](auto o) MNN_INLINE {
    if (o < L.T[0]) c0[o] = *reinterpret_cast<const mnn_f4*>(lds + L.o_b0 + o * 16 + q * 4);
  });
  const float* const pw = lds + L.o_w0s + lane;  // (tile o, k-step s at o * ostride + 64 s: the k-step is an immediate offset of the read)
  const int ostride = L.ks * 64;
  mnn_for<16>([&](auto s) MNN_INLINE {
    if (s < L.ks) {
      mnn_for<TM>([&](auto o) MNN_INLINE {
        if (o < L.T[0]) c0[o] = __builtin_amdgcn_mfma_f32_16x16x4f32(pw[o * ostride + s * 64], sig[s], c0[o], 0, 0, 0);
      });
    }
  });
}

// sum over the four lanes (j, 0..3) that hold one element: the same value in all four, the same order everywhere
__device__ __forceinline__ float mnn_sum_q(float p) {
  p += __shfl_xor(p, 16, 64);
  p += __shfl_xor(p, 32, 64);
  return p;
}

// ELU(alpha = 1), and with its derivative
__device__ __forceinline__ float mnn_elu(float p) { return p > 0.f ? p : expm1f(p); }
__device__ __forceinline__ void mnn_elu(float p, float& v, float& d) {
  v = p > 0.f ? p : expm1f(p);
  d = p > 0.f ? 1.f : expf(p);
}

// the block copies `floats` (a multiple of 4) of a 16-byte aligned image into LDS; the caller's barrier follows
__device__ __forceinline__ void mnn_stage_image(float* lds, const float* __restrict__ image, int floats, int tid) {
  for (int i = tid * 4; i < floats; i += MNN_THREADS * 4) *reinterpret_cast<mnn_f4*>(lds + i) = *reinterpret_cast<const mnn_f4*>(image + i);
}

// out[g] = W in[g] (+ b for the first NB members) for G right-hand sides at once, the form of the forward kernels that run two wavefronts per SIMD:
// the A fragment of an (out tile, in tile) pair is read once and feeds 4 G products; out tiles go in pairs, so 2 G accumulator chains are independent
// and the second tile's reads are immediate offsets of the first's.  tin / tout tiles; the tiles of one out tile are consecutive in the image.  in[g] /
// out[g] are the tile arrays of member g: a [G][TM] array, an array of G pointers, or &tiles for a single member.
template <int TM, int G, int NB, class In, class Out>
__device__ __forceinline__ void mnn_matvec(const float* W, const float* B, int tin, int tout, int lane, int q, In in, Out out) {
  const int rowstride = tin * 256;
  mnn_for<TM / 2>([&](auto P) MNN_INLINE {
    constexpr int o0 = 2 * P, o1 = o0 + 1;
    if (o0 < tout) {
      const bool two = o1 < tout;
      const float* const p0 = W + o0 * rowstride + lane * 4;
      const float* const p1 = p0 + rowstride;
      mnn_for<G>([&](auto g) MNN_INLINE {
        out[g][o0] = mnn_f4{0.f, 0.f, 0.f, 0.f};
        out[g][o1] = mnn_f4{0.f, 0.f, 0.f, 0.f};
        if constexpr (g < NB) {
          out[g][o0] = *reinterpret_cast<const mnn_f4*>(B + o0 * 16 + q * 4);
          if (two) out[g][o1] = *reinterpret_cast<const mnn_f4*>(B + o1 * 16 + q * 4);
        }
      });
      mnn_for<TM>([&](auto it) MNN_INLINE {
        if (it < tin) {
          const mnn_f4 a0 = *reinterpret_cast<const mnn_f4*>(p0 + it * 256);
          mnn_for<4>([&](auto r) MNN_INLINE {
            mnn_for<G>([&](auto g) MNN_INLINE { out[g][o0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[(int)r], in[g][it][(int)r], out[g][o0], 0, 0, 0); });
          });
          if (two) {
            const mnn_f4 a1 = *reinterpret_cast<const mnn_f4*>(p1 + it * 256);
            mnn_for<4>([&](auto r) MNN_INLINE {
              mnn_for<G>([&](auto g) MNN_INLINE { out[g][o1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[(int)r], in[g][it][(int)r], out[g][o1], 0, 0, 0); });
            });
          }
        }
      });
    }
  });
}

// ---- host ----------------------------------------------------------------------------------------
// ladj[n] = the columns of row n of e[N, D] added left to right, on `st` (csrc/mnn.hip holds the library's one kernel for it)
int mnn_rowsum(const float* e, float* out, long long N, int D, hipStream_t st);

// The launch geometry of an [N, Dsel] call: enough blocks for 256 CUs first, then longer runs per image load.  A pure function of the two sizes.
static inline int mnn_geometry(long long N, long long Dsel, int* rows_per_block, int* feats_per_block) {
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

// From an argument block P (zk_mnn_args_v1 / zk_umnn_args_v1: include/zuko_amd.h) to the kernel's arguments A (MnnArgs / UmnnArgs) and its grid, for the
// fields the two families name alike; `own(*p)` says whether the family's other fields are in range, and the family copies those itself.  Returns
// ZK_EINVAL for every refusal, otherwise 0; N == 0 is accepted before any pointer is examined and leaves grid->x == 0: nothing to launch.
template <bool INVERSE, class P, class A, class Own> static inline int mnn_prepare(const P* p, A* a, dim3* grid, Own own) {
  *grid = dim3(0);
  if (!p || p->struct_size != sizeof(P) || p->version != 1) return ZK_EINVAL;
  const int widths[3] = {p->width0, p->width1, p->width2};
  if (!mnn_layout(p->S, p->n_hidden, widths, &a->L)) return ZK_EINVAL;
  if (p->image_floats != a->L.total || p->n_features < 1 || p->N < 0 || p->Dsel < 1 || p->Dsel > (1 << 20)) return ZK_EINVAL;
  if (p->ldx < 1 || p->ldy < p->Dsel || !own(*p)) return ZK_EINVAL;
  if (INVERSE && (p->n_bisect < 0 || p->n_bisect > 64 || !(p->bound > 0))) return ZK_EINVAL;
  if (p->N == 0) return 0;
  if (!p->x || !p->signal || !p->image || !p->y) return ZK_EINVAL;
  if (!INVERSE && (!p->ladj || (p->ladj_reduced && !p->work))) return ZK_EINVAL;
  a->x = (const float*)p->x; a->signal = (const float*)p->signal; a->image = (const float*)p->image; a->feat = (const int*)p->feat;
  a->y = (float*)p->y; a->ladj = (float*)(p->ladj_reduced ? p->work : p->ladj);
  a->N = p->N; a->ldx = p->ldx; a->lds = p->ld_signal; a->ldy = p->ldy;
  a->Dsel = (int)p->Dsel; a->n_features = p->n_features; a->n_bisect = p->n_bisect; a->bound = (float)p->bound;
  if (mnn_geometry(a->N, a->Dsel, &a->rows_per_block, &a->feats_per_block) != 0) return ZK_EINVAL;  // (results do not depend on it)
  const long long cols = (a->Dsel + a->feats_per_block - 1) / a->feats_per_block;
  const long long gx = (a->N + a->rows_per_block - 1) / a->rows_per_block;
  if (gx > 0x7fffffffLL || cols > 65535) return ZK_EINVAL;
  *grid = dim3((unsigned)gx, (unsigned)cols);
  return 0;
}

// Grant, launch of MNN_THREADS-wide blocks over the kernel's one argument `args`, check — as ar_launch_dyn_lds of csrc/zk_ar_common.h (whose signature
// is tied to ArArgs and a one-dimensional grid); the grant is grant_dyn_lds of zk_common.h.
static inline int mnn_launch_dyn_lds(const void* fn, dim3 grid, int lds_bytes, void* args, hipStream_t st) {
  hipError_t e = grant_dyn_lds(fn, lds_bytes);
  if (e != hipSuccess) return (int)e;
  void* kargs[] = {args};
  e = hipLaunchKernel(fn, grid, dim3(MNN_THREADS), kargs, lds_bytes, st);
  if (e != hipSuccess) return (int)e;
  return ZK_LAUNCH_CHECK();
}

}  // namespace zk
