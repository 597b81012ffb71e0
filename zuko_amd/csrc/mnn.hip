// zuko_amd — monotone neural network of the neural autoregressive flow (NAF): value, derivative and bisection inverse.
//
// Replaces MNN.f + MonotonicTransform.call_and_ladj (zuko/flows/neural.py:56-71, zuko/transforms.py:623-637, zuko/nn.py:321-392):
//     y = MonotonicMLP_f(cat(x, signal));  ladj = log dy/dx          (the reference: stacked einsums + torch.autograd.grad)
// and MonotonicTransform._inverse + Bisection.forward (zuko/transforms.py:609-617, zuko/utils.py:170-178).  Every feature f owns a
// small network (1 + S) -> H1 [-> H2 [-> H3]] -> 1 with weights |W| and the two-way ELU; it runs once per element (n, d).
//
// Execution model (gfx950):
//   * a wavefront owns 16 elements of ONE feature for the whole network.  Every layer is computed transposed, H^T = |W| X^T, on
//     v_mfma_f32_16x16x4_f32 (exact fp32): A = a 16 x 4 slice of |W| (rows = out units), B = a 4 x 16 slice of the activations
//     (columns = elements).  Lane (j, q) = (lane & 15, lane >> 4) of the D fragment holds out units 16 t + 4 q + r (r = 0..3) of
//     element j — which is what the next layer wants as its B operand once its K axis is enumerated as k-step r <-> units
//     {r, 4 + r, 8 + r, 12 + r} of a 16-unit tile (the trick of csrc/fused_ar.hip): the weight image is laid out in that order, so
//     activations stay in registers from the signal load to log dy/dx.
//   * the derivative is carried in forward mode: the tangent enters as the column |w0[:, 0]| (no product needed), later layers
//     multiply it by the same |W_l| fragment as the value (two accumulators per A operand) and scale by act'(pre).
//   * the signal's share of the first layer, |W0[:, 1:]| signal + b0, is one short product per element; the bisection re-uses it
//     in every one of its steps.
//   * one feature's weight image (zuko_amd/mnn_plan.py: layout) sits in LDS, shared by the block's 4 wavefronts; a block covers
//     rows_per_block rows x feats_per_block consecutive columns and walks its columns one image at a time, so the lines of x and
//     of the signal a block touches are consumed by that block.  Nothing is staged through LDS besides the image.
//   * the two-way ELU and its derivative run on the vector unit; the last layer (H -> 1) is a per-lane dot product and two
//     cross-lane adds in a fixed order.  No atomics: ladj[N] is a second launch that adds the columns of a row in order.
//
// An element's y / ladj depends on its own x, signal and feature only: not on N, Dsel, the launch geometry or its neighbours.
#include "zk_mnn_common.h"

namespace zk {

struct MnnArgs {
  const float* x;       // forward: x; inverse: the targets
  const float* signal;
  const float* image;
  const int* feat;
  float* y;             // forward: y; inverse: the solutions
  float* ladj;          // [N, Dsel] (the per-element buffer, also when the caller asked for the row sums)
  long long N, ldx, lds, ldy;
  int Dsel, n_features, rows_per_block, feats_per_block, n_bisect;
  float bound;
  MnnLayout L;
};

// two-way ELU (zuko/nn.py:335-353): units below `half` take ELU(p), the others -ELU(-p); d = its derivative
__device__ __forceinline__ void mnn_act(float p, bool first, float& v, float& d) {
  float a;
  mnn_elu(first ? p : -p, a, d);
  v = first ? a : -a;
}
__device__ __forceinline__ float mnn_act(float p, bool first) {
  const float a = mnn_elu(first ? p : -p);
  return first ? a : -a;
}

// one hidden-to-hidden layer: v <- act(|W| v + b), t <- act'(.) * (|W| t); tin / tout tiles, `half` = ceil(width / 2)
template <int TM, bool TAN>
__device__ __forceinline__ void mnn_hidden(const float* W, const float* B, int tin, int tout, int half, int lane, int q, mnn_f4 (&v)[TM], mnn_f4 (&t)[TM]) {
  mnn_f4 ov[TM], ot[TM];
  const mnn_f4* const in[2] = {v, t};
  mnn_f4* const out[2] = {ov, ot};
  mnn_matvec<TM, TAN ? 2 : 1, 1>(W, B, tin, tout, lane, q, in, out);
  mnn_for<TM>([&](auto o) MNN_INLINE {
    if (o < tout) {
      mnn_for<4>([&](auto r) MNN_INLINE {
        const bool first = o * 16 + q * 4 + r < half;
        if constexpr (TAN) {
          float a, d;
          mnn_act(ov[o][(int)r], first, a, d);
          v[o][(int)r] = a;
          t[o][(int)r] = d * ot[o][(int)r];
        } else {
          v[o][(int)r] = mnn_act(ov[o][(int)r], first);
        }
      });
    }
  });
}

// the network behind the first layer's pre-activation: (y[, dy/dx]) of the element this lane belongs to
template <int TM, bool TAN>
__device__ __forceinline__ void mnn_tail(const MnnLayout& L, const float* lds, int lane, int q, float x, const mnn_f4 (&c0)[TM], float& y, float& dy) {
  mnn_f4 v[TM], t[TM];
  const int half0 = (L.T[0] * 16 + 1) / 2;
  mnn_for<TM>([&](auto o) MNN_INLINE {
    if (o < L.T[0]) {
      const mnn_f4 w = *reinterpret_cast<const mnn_f4*>(lds + L.o_w0x + o * 16 + q * 4);
      mnn_for<4>([&](auto r) MNN_INLINE {
        const float pre = fmaf(w[(int)r], x, c0[o][(int)r]);
        const bool first = o * 16 + q * 4 + r < half0;
        if constexpr (TAN) {
          float a, d;
          mnn_act(pre, first, a, d);
          v[o][(int)r] = a;
          t[o][(int)r] = d * w[(int)r];
        } else {
          v[o][(int)r] = mnn_act(pre, first);
        }
      });
    }
  });
  if (L.nh > 1) mnn_hidden<TM, TAN>(lds + L.o_w[1], lds + L.o_b[1], L.T[0], L.T[1], (L.T[1] * 16 + 1) / 2, lane, q, v, t);
  if (L.nh > 2) mnn_hidden<TM, TAN>(lds + L.o_w[2], lds + L.o_b[2], L.T[1], L.T[2], (L.T[2] * 16 + 1) / 2, lane, q, v, t);
  const int tl = L.T[L.nh - 1];
  float py = 0.f, pd = 0.f;
  mnn_for<TM>([&](auto o) MNN_INLINE {
    if (o < tl) {
      const mnn_f4 w = *reinterpret_cast<const mnn_f4*>(lds + L.o_wl + o * 16 + q * 4);
      mnn_for<4>([&](auto r) MNN_INLINE {
        py = fmaf(w[(int)r], v[o][(int)r], py);
        if constexpr (TAN) pd = fmaf(w[(int)r], t[o][(int)r], pd);
      });
    }
  });
  y = mnn_sum_q(py) + lds[L.o_bl];
  if constexpr (TAN) dy = mnn_sum_q(pd);
}

extern __shared__ __attribute__((aligned(16))) float mnn_lds[];

template <int TM, bool INVERSE> __global__ __launch_bounds__(MNN_THREADS, 2) void mnn_kernel(MnnArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
  const MnnLayout& L = a.L;
  const long long row0 = (long long)blockIdx.x * a.rows_per_block;
  for (int fc = 0; fc < a.feats_per_block; ++fc) {
    const int col = blockIdx.y * a.feats_per_block + fc;
    if (col >= a.Dsel) break;  // (uniform over the block)
    int f = a.feat ? a.feat[col] : col;
    f = f < 0 ? 0 : (f >= a.n_features ? a.n_features - 1 : f);  // (a memory guard only: the caller checks the range, zuko_amd/ops.py: _mnn_feat)
    const float* img = a.image + (size_t)f * L.total;
    __syncthreads();  // the previous column's image is no longer read
    mnn_stage_image(mnn_lds, img, L.total, tid);
    __syncthreads();
    for (int tile = wave; tile * 16 < a.rows_per_block && row0 + tile * 16 < a.N; tile += MNN_THREADS / 64) {
      const long long row = row0 + tile * 16 + j;
      const long long rc = row < a.N ? row : a.N - 1;  // rows behind the end compute on the last row and store nothing
      const float xin = a.x[rc * a.ldx + col];
      mnn_f4 c0[TM];
      mnn_signal<TM>(L, mnn_lds, a.signal + rc * a.lds + (size_t)col * L.S, lane, q, c0);
      if constexpr (!INVERSE) {
        float y, dy;
        mnn_tail<TM, true>(L, mnn_lds, lane, q, xin, c0, y, dy);
        if (q == 0 && row < a.N) {
          a.y[row * a.ldy + col] = y;
          a.ladj[row * a.Dsel + col] = logf(dy);
        }
      } else {
        // zuko/utils.py:170-178 in fp32: n times c = (a + b) / 2, f(c) < y ? a = c : b = c; the answer is the last midpoint
        float lo = -a.bound, hi = a.bound;
        for (int it = 0; it < a.n_bisect; ++it) {
          const float c = (lo + hi) / 2;
          float fy, unused;
          mnn_tail<TM, false>(L, mnn_lds, lane, q, c, c0, fy, unused);
          const bool below = fy < xin;
          lo = below ? c : lo;
          hi = below ? hi : c;
        }
        if (q == 0 && row < a.N) a.y[row * a.ldy + col] = (lo + hi) / 2;
      }
    }
  }
}

// ladj[n] = the columns of row n added left to right
__global__ __launch_bounds__(256) void mnn_rowsum_kernel(const float* __restrict__ e, float* __restrict__ out, long long N, int D) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int d = 0; d < D; ++d) s += e[n * D + d];
  out[n] = s;
}

int mnn_rowsum(const float* e, float* out, long long N, int D, hipStream_t st) {
  hipLaunchKernelGGL(mnn_rowsum_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, e, out, N, D);
  return ZK_LAUNCH_CHECK();
}

template <bool INVERSE> static int mnn_launch(const zk_mnn_args_v1* p, void* stream) {
  MnnArgs a;
  dim3 grid;
  const int err = mnn_prepare<INVERSE>(p, &a, &grid, [](const zk_mnn_args_v1& b) { return b.ld_signal >= (int64_t)b.Dsel * b.S; });
  if (err != 0 || grid.x == 0) return err;
  hipStream_t st = (hipStream_t)stream;
  const bool small = a.L.T[0] <= 4 && a.L.T[1] <= 4 && a.L.T[2] <= 4;
  const void* fn = small ? (const void*)mnn_kernel<4, INVERSE> : (const void*)mnn_kernel<8, INVERSE>;
  const int rc = mnn_launch_dyn_lds(fn, grid, a.L.total * 4, &a, st);
  if (rc != 0 || INVERSE || !p->ladj_reduced) return rc;
  return mnn_rowsum((const float*)p->work, (float*)p->ladj, a.N, a.Dsel, st);
}

}  // namespace zk

extern "C" int zk_mnn_forward(const zk_mnn_args_v1* args, void* stream) { return zk::mnn_launch<false>(args, stream); }
extern "C" int zk_mnn_inverse(const zk_mnn_args_v1* args, void* stream) { return zk::mnn_launch<true>(args, stream); }
extern "C" int zk_mnn_launch_geometry(int64_t N, int64_t Dsel, int* rows_per_block, int* feats_per_block) { return zk::mnn_geometry(N, Dsel, rows_per_block, feats_per_block); }
extern "C" int zk_mnn_image_floats(int S, int n_hidden, int width0, int width1, int width2) {
  zk::MnnLayout L;
  const int widths[3] = {width0, width1, width2};
  return zk::mnn_layout(S, n_hidden, widths, &L) ? L.total : -1;
}
