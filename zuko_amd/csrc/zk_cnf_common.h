// zuko_amd — what the step kernel of the continuous flow (csrc/cnf.hip) and its adjoint (csrc/cnf_backward.hip) share: the layout of the field's
// weight image, the Dormand-Prince tableau, the time embedding (cnf_embed), the first layer's pre-activation (cnf_first_layer) and the checks both
// launchers make on t, dt, trace_scale and ld_pre (cnf_step_fields_ok).  The activation is mnn_elu of csrc/zk_mnn_common.h.  The last layer's product
// stands in both files (sharing it cost the adjoint registers: profiles/small_net_frame/census.md); the two __global__ bodies and their sweeps are
// each file's own.
#pragma once
#include "zk_mnn_common.h"
#include <math.h>

namespace zk {

// Offsets (floats) of the image; the same arithmetic as zuko_amd/cnf_plan.py: layout.
struct CnfLayout {
  int nh, F, Q, kt, kx;  // hidden layers, features, frequencies, k-steps of the time product = ceil(2 Q / 4) and of the x product = ceil(F / 4)
  int T[3];              // 16-unit tiles per hidden layer
  int o_fr, o_w0t, o_w0x, o_w0c, o_w[3], o_b[3], o_wo, o_bo, o_wl, total;
};

static inline bool cnf_layout(int F, int Q, int nh, const int* widths, CnfLayout* L) {
  if (F < 1 || F > 16 || Q < 1 || Q > 8 || nh < 1 || nh > 3) return false;
  for (int l = 0; l < 3; ++l) {
    const int h = widths[l];
    if (l < nh ? (h < 16 || h > 128 || h % 16 != 0) : h != 0) return false;
    L->T[l] = h / 16;
  }
  L->nh = nh; L->F = F; L->Q = Q; L->kt = (2 * Q + 3) / 4; L->kx = (F + 3) / 4;
  int o = 0;
  L->o_fr = o; o += 8;
  L->o_w0t = o; o += L->T[0] * L->kt * 64;
  L->o_w0x = o; o += L->T[0] * L->kx * 64;
  L->o_w0c = o; o += F * L->T[0] * 16;
  L->o_w[0] = L->o_b[0] = 0;
  for (int l = 1; l < 3; ++l) {
    L->o_w[l] = o; if (l < nh) o += L->T[l] * L->T[l - 1] * 256;
    L->o_b[l] = o; if (l < nh) o += L->T[l] * 16;
  }
  L->o_wo = o; o += L->T[nh - 1] * 256;
  L->o_bo = o; o += 16;
  L->o_wl = o; o += F * L->T[nh - 1] * 16;
  L->total = o;
  return o * 4 <= MNN_LDS_MAX;
}

// Dormand-Prince: stage s (0..6) is evaluated at t + CNF_C[s] dt on x + sum_m CNF_A[s][m] k_m; row 6 is the fifth-order result, whose field value is k_7
// of the embedded fourth-order one.  The quotients are rounded from double once, as a Python float times a float32 tensor is.  CNF_E holds the
// DIFFERENCE of the two results' weights: next - star = sum_m CNF_E[m] k_m is formed from the k directly.  The reference subtracts the two sums, which
// in float32 leaves the rounding of a dozen additions at the state's magnitude in a quantity a hundred thousand times smaller (its ratio moves by
// +-0.02 between two correct float32 evaluations); the direct sum is the same quantity without that cancellation.
static __constant__ float CNF_C[7] = {0.f, (float)(1.0 / 5), (float)(3.0 / 10), (float)(4.0 / 5), (float)(8.0 / 9), 1.f, 1.f};
static __constant__ float CNF_A[7][6] = {
    {0.f, 0.f, 0.f, 0.f, 0.f, 0.f},
    {(float)(1.0 / 5), 0.f, 0.f, 0.f, 0.f, 0.f},
    {(float)(3.0 / 40), (float)(9.0 / 40), 0.f, 0.f, 0.f, 0.f},
    {(float)(44.0 / 45), -(float)(56.0 / 15), (float)(32.0 / 9), 0.f, 0.f, 0.f},
    {(float)(19372.0 / 6561), -(float)(25360.0 / 2187), (float)(64448.0 / 6561), -(float)(212.0 / 729), 0.f, 0.f},
    {(float)(9017.0 / 3168), -(float)(355.0 / 33), (float)(46732.0 / 5247), (float)(49.0 / 176), -(float)(5103.0 / 18656), 0.f},
    {(float)(35.0 / 384), 0.f, (float)(500.0 / 1113), (float)(125.0 / 192), -(float)(2187.0 / 6784), (float)(11.0 / 84)},
};
static __constant__ float CNF_E[7] = {(float)(35.0 / 384 - 5179.0 / 57600), 0.f, (float)(500.0 / 1113 - 7571.0 / 16695), (float)(125.0 / 192 - 393.0 / 640),
                                      (float)(92097.0 / 339200 - 2187.0 / 6784), (float)(11.0 / 84 - 187.0 / 2100), -(float)(1.0 / 40)};

// element e of the time embedding (cos(fr ts), sin(fr ts)) of the image's Q frequencies; zero behind 2 Q
__device__ __forceinline__ float cnf_embed(const CnfLayout& L, const float* lds, int e, float ts) {
  const float arg = lds[L.o_fr + (e < L.Q ? e : (e < 2 * L.Q ? e - L.Q : 0))] * ts;
  return e < L.Q ? cosf(arg) : (e < 2 * L.Q ? sinf(arg) : 0.f);
}

// tile o of the first layer's pre-activation of the wave's rows: pre + W0t emb + W0x x
__device__ __forceinline__ mnn_f4 cnf_first_layer(const CnfLayout& L, const float* lds, const float* __restrict__ prow, int lane, int q, int o, const float (&emb)[4],
                                                  const float (&xin)[4]) {
  const float* const pt = lds + L.o_w0t + lane;
  const float* const px = lds + L.o_w0x + lane;
  mnn_f4 c = *reinterpret_cast<const mnn_f4*>(prow + o * 16 + q * 4);
  mnn_for<4>([&](auto s) MNN_INLINE {
    if (s < L.kt) c = __builtin_amdgcn_mfma_f32_16x16x4f32(pt[(o * L.kt + s) * 64], emb[s], c, 0, 0, 0);
  });
  mnn_for<4>([&](auto s) MNN_INLINE {
    if (s < L.kx) c = __builtin_amdgcn_mfma_f32_16x16x4f32(px[(o * L.kx + s) * 64], xin[s], c, 0, 0, 0);
  });
  return c;
}

// ---- host ----------------------------------------------------------------------------------------
// what both launchers ask of the fields their argument blocks (zk_cnf_args_v1 / zk_cnf_adj_args_v1) name alike; `traced`: trace_scale is used
template <class P> static inline bool cnf_step_fields_ok(const P* p, bool traced) {
  if (p->ld_pre != 0 && (p->ld_pre < p->width0 || p->ld_pre % 4 != 0)) return false;
  if (!std::isfinite(p->t) || !std::isfinite(p->dt)) return false;
  return !traced || (p->trace_scale > 0 && std::isfinite(p->trace_scale));
}

}  // namespace zk
