// zuko_amd — the FRAME shared by the fused autoregressive kernels (fused_ar.hip, fused_ar_gsplit.hip: the generic kernels; fused_ar_static_impl.h,
// fused_ar_split_impl.h, fused_ar_half_impl.h: the templates of the generated static-shape kernels): launch arguments, LDS layout, lane
// decomposition, table staging, the input stage (non-finite flag, row tiles), activations, the per-group operand fetch, the univariate epilogue,
// the running log-derivative and the host's grant-and-launch tail.  The kernel files hold their matrix parts (block loops, operand split, waits).
#pragma once
#include "zk_univariate.h"
#include <cstddef>
#include <cstring>

namespace zk {

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define AR_TF 256 /* floats per tile image */
#define AR_WAVES 8
#define AR_T 16   /* activation tiles (256 units) */
#define ARS_ABI 10 /* contract between this library and the generated static-shape kernels (zuko_amd/static_ar.py): bump on any change of ArArgs */
#ifndef ARX_ABL
#define ARX_ABL 0  // timing ablations of the operand-split kernel (scripts/split_ablate.py): 1 no DMA, 2 no MFMA, 3 no epilogue, 4 no barrier, 5 no LDS reads, 6 no conversions
#endif
#ifndef ARH_POISON_ONE
#define ARH_POISON_ONE 1  // probe builds: 0 = the NaN-or-zero is added to all K search-axis parameters of a spline (UniRqs::poison)
#endif

struct ArArgs {
  int64_t N;
  int D, DIN;               // features, conditioner inputs (features + context), DIN % 4 == 0
  const float* x; int64_t ldx;  // [N, DIN] = cat(x, c) zero-padded to a multiple of 4; rows 16-byte aligned
  float* y; int64_t ldy;
  const float* yin; int64_t ldyin;  // INVERSE only: the values to invert (y of the forward map)
  float* ladj; int accumulate;
  const float* stream;
  const float* bias;
  const uint32_t* skip;
  const int32_t* featmap;
  int L, NG, n_chunks, act, bias_floats, dbg;
  const int* sched;  // optional chunk schedule (partial inverse sweeps): stream chunk ids in consumption order
  int n_sched;
  int olim[8];       // per hidden layer: last out-group (of 4 tiles) to evaluate; 3 = all
  int g0, g1;        // last-layer groups [g0, g1) to evaluate
  int xlds;  // x (or y_in) and the result tile are staged in a wave-private LDS region (stride xs words)
  int xs;
  float bound, ls;
  RqsLeanConst lc;   // spline epilogues: constants of rqs_lean
  int64_t n_tiles;
  int32_t* bin_out;  // diagnostic instantiation only: bin index [N, D] and the K+1 search-axis knots [N, D, K+1]
  float* knots_out;
  int l1rev;         // static-shape kernels only: the first layer follows the pattern's ALTERNATIVE input tiles (descending feature order)
  // static-shape kernels, conditioner-only (training) instantiation: the hidden activations [N, width_l] (units in the stream's
  // sorted order) and the packed parameters phi [N, D * total] (module order) are written out; y / ladj are not
  float* act_out[3];
  float* phi_out;
  int64_t ldphi;
  // static-shape dgrad chain (ars_dgrad_kernel): saved activations h_l [N, width_l] whose sign gates the gradient of layer l
  const float* gate[3];
  // fused backward of an autoregressive transform (arxb_kernel): x / featmap as for the forward; the forward's phi and the gradient
  // of phi it writes for the weight gradients [N, D * total] (row stride ldpin); gy [N, D] (row stride ldgy), gl [N]; the input gradient
  // goes to phi_out (row stride ldphi) as in the dgrad chain
  const float* phi_in;
  float* gphi_out;
  int64_t ldpin;
  const float* gy; int64_t ldgy;
  const float* gl;
  // training launches: phi (and its gradient) in the kernels' PACKED order instead of the module's — row n holds, for group g and tile t,
  // 16 floats at (g NT + t) 16: parameter 4 t + r of the features of lane q = 0..3 at 4 q + r (row stride >= NG * NT * 16), which is
  // how a lane holds them in registers: 16-byte accesses, no regrouping (zuko_amd/train.py keeps such a phi to itself)
  int phi_packed;
  // polynomial maps (uni_kind 5, 6; operand-split static-shape kernels only): constants of the SOS quadrature, Bernstein continuation margin
  SosConst<float> sos;
  float eps;
  // two-part (f16) operand-split kernels (fused_ar_half_impl.h): 2^-ew_l of every linear layer, the power of two its weights were stored with
  float wdescale[4];
  // training launches (operand-split static-shape kernels): where to fold the maximum magnitude of every tensor the launch stores for the weight
  // gradients (zk_half.h: 64 slots) — forward: amax[l] for act_out[l]; backward: amax[l] for act_out[l] (gradient of a hidden layer), amax[3] for
  // gphi_out.  null = not wanted.  With them the weight gradients run on two-part f16 operands (csrc/train.hip: wgrad_split_body<true>).
  unsigned* amax[4];
  // terminal launch of a log_prob (operand-split static-shape kernels: arht_kernel, arxt_kernel): loc [D] and scale [D] of the diagonal-normal base.
  // base_loc != null: y is NOT written, and ladj receives (ladj +) log|dy/dx| + sum_f log N(y_f; loc_f, scale_f) — the log-density itself
  const float* base_loc;
  const float* base_scale;
};

// Second argument of the two-part kernels' FLOW launch (fused_ar_half_impl.h: arhf_kernel — all T transforms of a composed flow in one launch):
// what differs per transform.  ArArgs::stream then holds the T streams back to back (ArArgs::n_chunks chunks each).
struct ArhFlow {
  int T;                   // transforms
  int bias_stride;         // floats between two bias images in `bias`: whole 1 KiB pieces, >= ArArgs::bias_floats
  int n_fmaps;             // distinct feature maps in `featmap`, NG * 4 * FPL words each
  int term;                // set by the launcher: the last pass ends in the base's log-density (ArArgs::base_loc), no y
  const float* bias;       // T bias images
  const int32_t* featmap;
  const float* table;      // per transform 8 words: the four descale factors of its stream (float), the index of its feature map (int), first layer on the alternative pattern (int), 2 unused
};
// launcher of the flow kernel exported by a generated two-part unit (zuko_amd/static_ar.py: FLOW_ENTRY)
typedef int (*arhf_launch_fn)(const ArArgs* a, const ArhFlow* f, int abi, int args_bytes, int flow_bytes, void* stream);

__device__ __forceinline__ float act_f32(float v, int act) {
  switch (act) {
    case 1: return v < 0.f ? 0.f : v;
    case 2: return v > 0.f ? v : expm1f(v);
    case 3: return tanhf(v);
    case 4: return v / (1.f + expf(-v));
    case 5: return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
    case 6: return 1.f / (1.f + expf(-v));
    case 7: return v > 0.f ? v : 0.01f * v;
    default: return v;
  }
}


// ---- univariate epilogues -------------------------------------------------------------------------
struct UniAffine {
  static constexpr int TOTAL = 2, FPL = 2, NT = 1;
  template <bool INV> static __device__ __forceinline__ void poison(float* p, int base, float nan_or_zero) {
    p[base + 0] += nan_or_zero;
    p[base + 1] += nan_or_zero;
  }
  static constexpr int NKNOT = 1;
  template <typename P, typename A> static __device__ __forceinline__ void fwd(const P& p, int base, const A& a, float x, float& y, float& lj, int* k = nullptr, float* ks = nullptr) {
    affine_fwd<float, MathFast>(p(base + 0), p(base + 1), a.ls, x, y, lj);
  }
  template <typename P, typename A> static __device__ __forceinline__ float inv(const P& p, int base, const A& a, float y) {
    return affine_inv<float, MathFast>(p(base + 0), p(base + 1), a.ls, y);
  }
};

// K-bin rational-quadratic spline; CIRC: preceded by the circular shift of NCSF (zuko/flows/spline.py:65-72,
// zuko/transforms.py:344-348: x -> remainder(x, 2B) - B with B = pi passed as `bound`).
template <int K, bool CIRC> struct UniRqs {
  static constexpr int TOTAL = 3 * K - 1, FPL = 1, NT = (TOTAL + 3) / 4;
  static __device__ __forceinline__ float shift(float v, float bound) {
    const float period = 2.f * bound;
    float r = fmodf(v, period);
    r = (r < 0.f) ? r + period : r;  // torch.remainder: result takes the sign of the divisor
    return r - bound;
  }
  // All-NaN parameters (reference: zuko/nn.py:217-218 on a non-finite input) leave knot 0 = -B finite and every other
  // knot NaN: values right of -B land in bin 0 with a NaN corner (y = NaN), values at or left of it, NaN and -inf keep
  // y = v, and log|dy/dx| is NaN everywhere.  NaN widths (heights for the inverse, which searches the other axis) give
  // exactly that: the remaining parameters never reach an output that is not already NaN.  ONE add is enough: the knots
  // are a running sum (rqs_lean: acc += 2^(u_j r_j), cum[j] = acc) that turns NaN at j = 0 and stays NaN, and the
  // normaliser 1 / acc is NaN with it, so knots 1 .. K come out NaN whatever parameters 1 .. K - 1 hold.
  template <bool INV> static __device__ __forceinline__ void poison(float* p, int base, float nan_or_zero) {
#if ARH_POISON_ONE
    p[base + (INV ? K : 0)] += nan_or_zero;
#else
#pragma unroll
    for (int j = 0; j < K; ++j) p[base + (INV ? K : 0) + j] += nan_or_zero;
#endif
  }
  static constexpr int NKNOT = K + 1;
  // k / ks (diagnostic instantiation): bin index and search-axis knots of THIS evaluation
  template <typename P, typename A> static __device__ __forceinline__ void fwd(const P& p, int base, const A& a, float x, float& y, float& lj, int* k = nullptr, float* ks = nullptr) {
    int kk;
    rqs_lean<K, false>([&](int j) { return p(base + j); }, [&](int j) { return p(base + K + j); }, [&](int j) { return p(base + 2 * K + j); }, a.lc,
                       CIRC ? shift(x, a.bound) : x, y, lj, kk, ks);
    if (k) *k = kk;
  }
  template <typename P, typename A> static __device__ __forceinline__ float inv(const P& p, int base, const A& a, float y) {
    float x, lj;
    rqs_lean<K, true>([&](int j) { return p(base + j); }, [&](int j) { return p(base + K + j); }, [&](int j) { return p(base + 2 * K + j); }, a.lc, y, x, lj);
    return CIRC ? shift(x, a.bound) : x;
  }
};
// Shifted sum-of-squares polynomial (zuko/transforms.py:905-963 + the learned constant of zuko/flows/polynomial.py:64-70): P polynomials of L1
// coefficients, then the shift.  FORWARD only (the inverse is a bisection: it stays with the layer-wise kernels).
template <int P, int L1> struct UniSos {
  static constexpr int TOTAL = P * L1 + 1, FPL = 1, NT = (TOTAL + 3) / 4, NKNOT = 1;
  template <bool INV> static __device__ __forceinline__ void poison(float* p, int base, float nan_or_zero) {
    p[base] += nan_or_zero;             // (a NaN coefficient makes f and g NaN: y and log|dy/dx| NaN, as the reference's all-NaN parameters do)
    p[base + P * L1] += nan_or_zero;
  }
  template <typename Pa, typename A> static __device__ __forceinline__ void fwd(const Pa& p, int base, const A& a, float x, float& y, float& lj, int* k = nullptr, float* ks = nullptr) {
    auto ld = [&](int j) { return p(base + j); };
    y = sos_f<float>(Fixed<P>{}, Fixed<L1>{}, a.sos, ld, x) + p(base + P * L1);
    lj = t_log(sos_g<float>(Fixed<P>{}, Fixed<L1>{}, a.sos, ld, x));
  }
};
// Bounded Bernstein polynomial (zuko/transforms.py:779-831) with NC - 5 unconstrained parameters.  FORWARD only.
template <int NC> struct UniBernBounded {
  static constexpr int TOTAL = NC - 5, FPL = 1, NT = (TOTAL + 3) / 4, NKNOT = 1;
  template <bool INV> static __device__ __forceinline__ void poison(float* p, int base, float nan_or_zero) { p[base] += nan_or_zero; }  // (softmax: one NaN makes every coefficient NaN)
  template <typename Pa, typename A> static __device__ __forceinline__ void fwd(const Pa& p, int base, const A& a, float x, float& y, float& lj, int* k = nullptr, float* ks = nullptr) {
    float th[NC];
    bern_theta_bounded<float>(Fixed<NC>{}, [&](int j) { return p(base + j); }, a.bound, th);
    const BernTails<float> t = bern_tails<float>(Fixed<NC>{}, th, true, a.bound, a.eps);
    float d;
    bern_fwd<float>(Fixed<NC>{}, th, t, a.bound, x, y, d, a.eps);
    lj = t_log(d);
  }
};
typedef UniSos<3, 5> UniSos3x5;            // SOSPF defaults (zuko/flows/polynomial.py:51-53)
typedef UniBernBounded<22> UniBern17;      // BPF default degree 16 (zuko/flows/polynomial.py:97)
typedef UniRqs<8, false> UniRqs8;
typedef UniRqs<4, false> UniRqs4;
typedef UniRqs<16, false> UniRqs16;
typedef UniRqs<8, true> UniCircRqs8;


// ---- the frame ------------------------------------------------------------------------------------
// LDS of a forward kernel:  ring | bias image | feature map | skip words | wave-private row tiles (16 samples x xs words per wavefront, XLDS only).
// ONE definition for the kernels (the carved pointers) and their launchers (the size; the limits on feature groups and skip words).
struct ArLds {
  static constexpr int FMAP_WORDS = 1024, SKIP_WORDS = 256;  // (1024 + 256 words between the bias image and the row tiles)
  static constexpr int bytes(int ring_floats, int bias_floats, int row_waves, int xs) {  // row_waves: wavefronts that stage rows (0: none)
    return (ring_floats + bias_floats + FMAP_WORDS + SKIP_WORDS + row_waves * 16 * xs) * (int)sizeof(float);
  }
  // the carved pointers, each from the one before it (the bias image starts right behind the ring)
  static __device__ __forceinline__ int* fmap(float* bias, int bias_floats) { return reinterpret_cast<int*>(bias + bias_floats); }
  static __device__ __forceinline__ int* skip(int* fmap_) { return fmap_ + FMAP_WORDS; }
  static __device__ __forceinline__ float* row(int* fmap_, int wave, int j, int xs) {  // this lane's sample row of its wavefront's tile
    return reinterpret_cast<float*>(fmap_ + FMAP_WORDS + SKIP_WORDS) + wave * 16 * xs + j * xs;
  }
  // cooperative copy of the launch's tables (n_skip words of a.skip from skip0 on: the generic kernels), then the workgroup barrier
  template <int THREADS> static __device__ __forceinline__ void stage(const ArArgs& a, int tid, float* bias, int* fmap_, int n_fmap, int skip0 = 0, int n_skip = 0) {
    for (int i = tid; i < a.bias_floats; i += THREADS) bias[i] = a.bias[i];
    for (int i = tid; i < n_fmap; i += THREADS) fmap_[i] = a.featmap[i];
    for (int i = tid; i < n_skip; i += THREADS) skip(fmap_)[i] = (int)a.skip[skip0 + i];
    __syncthreads();
  }
  // Terminal launch: three D-float tables behind the feature map's n_fmap words, indexed by FEATURE id — loc_f, 1 / (2 s_f^2) and
  // -log s_f - log sqrt(2 pi) — from the base's device buffers (they may change between calls: nothing is kept on the host).  Call in front of
  // stage(), whose barrier publishes them.  n_fmap + 3 D <= FMAP_WORDS is the launcher's to check (base_fits).
  static constexpr bool base_fits(int n_fmap, int D) { return n_fmap + 3 * D <= FMAP_WORDS; }
  static __device__ __forceinline__ float* base(int* fmap_, int n_fmap) { return reinterpret_cast<float*>(fmap_ + n_fmap); }
  template <int THREADS> static __device__ __forceinline__ void stage_base(const ArArgs& a, int tid, float* tab, int D) {
    for (int i = tid; i < D; i += THREADS) {
      const float s = a.base_scale[i];
      tab[i] = a.base_loc[i];
      tab[D + i] = 1.f / (2.f * (s * s));
      tab[2 * D + i] = -t_log(s) - 0.91893853320467274178f;
    }
  }
};

// a wavefront owns 16 samples: lane (j, q) holds units 4 q .. 4 q + 3 of every 16-unit tile of sample j
struct ArLane {
  int tid, lane, wave, j, q;
  __device__ __forceinline__ ArLane() : tid(threadIdx.x), lane(tid & 63), wave(__builtin_amdgcn_readfirstlane(tid >> 6)), j(lane & 15), q(lane >> 4) {}
};

// A NaN / inf input turns ALL parameters of its sample into NaN in the reference (it multiplies every input by mask * W: x * 0 = NaN, zuko/nn.py:217-218),
// including those whose mask excludes that input.  Skipped tiles would not reproduce that, so the sample is flagged: NaN for such a sample, else 0.
template <int NIT, int M> __device__ __forceinline__ float ar_poison_of(const f32x4 (&v)[M]) {
  int bad = 0;
#pragma unroll
  for (int it = 0; it < NIT; ++it)
#pragma unroll
    for (int r = 0; r < 4; ++r) bad |= !(fabsf(v[it][r]) < __builtin_inff());
  bad |= __shfl_xor(bad, 16, 64);
  bad |= __shfl_xor(bad, 32, 64);
  return bad ? __builtin_nanf("") : 0.f;
}

// The wave-private [16 samples x D] row tile: the epilogue's input values on the way in, the results on the way out.  It keeps the per-group operand
// fetch on the LDS (lgkmcnt) queue — a global load there would wait behind the ring DMAs in flight — and turns 4-byte scattered result stores into
// 16-byte row stores.  (Static-shape kernels: D at compile time.  The two generic kernels bound the columns by the run-time a.D in place: as shared
// helpers these loops moved their register allocation, profiles/ar_frame/census.md.)
template <int D, int M> __device__ __forceinline__ void ar_rows_in(float* xr, int q, const f32x4 (&v)[M]) {
#pragma unroll
  for (int it = 0; it < (D + 15) / 16; ++it)
    if ((it + 1) * 16 <= D || it * 16 + 4 * q < D) *reinterpret_cast<f32x4*>(xr + it * 16 + 4 * q) = v[it];
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}
template <int D> __device__ __forceinline__ void ar_rows_out(const float* xr, int q, float* yrow, bool live) {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  if (live) {
#pragma unroll
    for (int it = 0; it < (D + 15) / 16; ++it)
      if ((it + 1) * 16 <= D || it * 16 + 4 * q < D) *reinterpret_cast<f32x4*>(yrow + it * 16 + 4 * q) = *reinterpret_cast<const f32x4*>(xr + it * 16 + 4 * q);
  }
}
// Activation between the layers of a static-shape kernel, dst = act(src) over N tiles (dst may be src; the generic kernels switch on the run-time id).  ELU / tanh / SiLU / GELU / sigmoid / leaky ReLU sit inside a loop the
// compiler must not unroll over the activation's inline expansion (64-128 copies of tanhf / erff made the epilogue instruction-cache bound).
template <int ACT, int N, int M> __device__ __forceinline__ void ar_activate(f32x4 (&dst)[M], const f32x4 (&src)[M]) {
  if constexpr (ACT == 1) {
#pragma unroll
    for (int t = 0; t < N; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[t][r] = src[t][r] < 0.f ? 0.f : src[t][r];  // NaN stays NaN, as torch.relu
  } else if constexpr (ACT == 0) {
#pragma unroll
    for (int t = 0; t < N; ++t) dst[t] = src[t];
  } else {
#pragma unroll 1
    for (int rep = 0; rep < 1; ++rep) {
#pragma unroll
      for (int t = 0; t < N; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[t][r] = act_f32(src[t][r], ACT);
    }
  }
}
// Feature ids of this lane's slots in every group of the last layer.  REGS: constant over the launch, kept in registers when they fit (a per-group
// LDS read puts one exposed LDS round trip in front of the read of x that depends on it).
template <int NG, int FPL, bool REGS> struct ArFids {
  int r[REGS ? NG * FPL : 1];
  const int* fmap;
  int q;
  __device__ __forceinline__ ArFids(const int* fmap_lds, int q_) : fmap(fmap_lds), q(q_) {
    if constexpr (REGS) {
#pragma unroll
      for (int i = 0; i < NG; ++i)
#pragma unroll
        for (int fi = 0; fi < FPL; ++fi) r[i * FPL + fi] = fmap[(i * 4 + q) * FPL + fi];
    }
  }
  // operands of group g's epilogue, requested before the group's matrix instructions: feature ids, then x from the row tile (XLDS) or the global row
  template <bool XLDS> __device__ __forceinline__ void fetch(int g, const float* xr, const float* xrow, int (&fid)[FPL], float (&xin)[FPL]) const {
#pragma unroll
    for (int fi = 0; fi < FPL; ++fi) {
      if constexpr (REGS) fid[fi] = r[g * FPL + fi];
      else fid[fi] = fmap[(g * 4 + q) * FPL + fi];
      const int fc = fid[fi] < 0 ? 0 : fid[fi];
      if constexpr (XLDS) xin[fi] = xr[fc];
      else xin[fi] = xrow[fc];
    }
  }
  // terminal launch: the base's table entries (ArLds::stage_base, D floats each) of the group's features, requested with the operands above
  __device__ __forceinline__ void fetch_base(const int (&fid)[FPL], const float* base, int D, float (&bv)[3 * FPL]) const {
#pragma unroll
    for (int fi = 0; fi < FPL; ++fi) {
      const int fc = fid[fi] < 0 ? 0 : fid[fi];
#pragma unroll
      for (int k = 0; k < 3; ++k) bv[3 * fi + k] = base[k * D + fc];
    }
  }
};

// The univariate map on the group's parameters p (registers) in the static-shape kernels: y to the row tile (XLDS) or straight to global memory,
// log|dy/dx| added to lacc.  ABL: the kernel honours the ARX_ABL == 3 ablation (the operand-split kernels; not the f32 one).  (The two generic kernels
// keep their epilogue in place — inverse branch, partial-sweep stores, timing probe — for the same reason as their row loops.)
// A sample with a non-finite input has NaN parameters throughout in the reference; making the parameters of the SEARCH axis NaN reproduces every
// output of that case (Uni::poison) at a third of the additions.  DIAG: the diagnostic twin — the bin index the spline USED and the knots it
// searched are stored as well (bin_out [N, D], knots_out [N, D, NKNOT]).  TERM: the terminal launch of a log_prob — y is not stored; the base's
// log-density of y_f (bv: loc_f, 1 / (2 s_f^2), -log s_f - log sqrt(2 pi) per slot, ArFids::fetch_base) joins log|dy/dx| in lacc.  A poisoned sample has lj = NaN for every feature, so its sum is NaN.
template <typename Uni, bool DIAG, bool XLDS, bool ABL = true, bool TERM = false>
__device__ __forceinline__ void ar_uni_epilogue(float (&p)[4 * Uni::NT], const ArArgs& a, const int (&fid)[Uni::FPL], const float (&xin)[Uni::FPL], float poison, float* xr, int64_t n,
                                                bool live, int D, float& lacc, const float* bv = nullptr) {
  constexpr int FPL = Uni::FPL, TOTAL = Uni::TOTAL;
#pragma unroll
  for (int fi = 0; fi < FPL; ++fi) Uni::template poison<false>(p, fi * TOTAL, poison);
  auto ld = [&](int i) { return p[i]; };
#pragma unroll
  for (int fi = 0; fi < FPL; ++fi) {
    const int f = fid[fi];
    if (f >= 0) {
      float yv, lj;
      if (ABL && ARX_ABL == 3) {
        yv = p[fi * TOTAL] + xin[fi]; lj = p[fi * TOTAL + 1];
#pragma unroll
        for (int i = 2; i < TOTAL; ++i) lj += p[fi * TOTAL + i];
      } else if constexpr (DIAG) {
        int kb = 0;
        float ks[Uni::NKNOT];
        Uni::fwd(ld, fi * TOTAL, a, xin[fi], yv, lj, &kb, ks);
        if (live) {
          a.bin_out[n * D + f] = kb;
#pragma unroll
          for (int jj = 0; jj < Uni::NKNOT; ++jj) a.knots_out[(n * D + f) * Uni::NKNOT + jj] = ks[jj];
        }
      } else Uni::fwd(ld, fi * TOTAL, a, xin[fi], yv, lj);
      if constexpr (TERM) {
        const float df = yv - bv[3 * fi];
        lacc += lj;
        lacc += __builtin_fmaf(-(df * df), bv[3 * fi + 1], bv[3 * fi + 2]);
      } else {
        if constexpr (XLDS) xr[f] = yv;
        else if (live) a.y[n * a.ldy + f] = yv;
        lacc += lj;
      }
    }
  }
}

// the sample's log|dy/dx|: summed over q with two shuffles, stored (or added to what the buffer holds — ladj_in when the caller requested it ahead)
template <bool PREFETCHED = false> __device__ __forceinline__ void ar_ladj_store(const ArArgs& a, float lacc, int64_t n, bool live, int q, float ladj_in = 0.f) {
  if (a.ladj) {
    lacc += __shfl_xor(lacc, 16, 64);
    lacc += __shfl_xor(lacc, 32, 64);
    if (live && q == 0) a.ladj[n] = a.accumulate ? (PREFETCHED ? ladj_in : a.ladj[n]) + lacc : lacc;
  }
}

// ---- host ----------------------------------------------------------------------------------------
// Grant (zk_common.h: grant_dyn_lds), launch, check.
static inline int ar_launch_dyn_lds(const void* fn, int max_grid, int block, int lds_bytes, ArArgs& a, void* stream) {
  hipError_t e = grant_dyn_lds(fn, lds_bytes);
  if (e != hipSuccess) return (int)e;
  const unsigned grid = (unsigned)(a.n_tiles < max_grid ? a.n_tiles : max_grid);
  void* kargs[] = {&a};
  e = hipLaunchKernel(fn, dim3(grid), dim3((unsigned)block), kargs, lds_bytes, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  return ZK_LAUNCH_CHECK();
}

// Versioned argument block (include/zuko_amd.h: zk_ar_args_v1 — every entry point checks struct_size / version before it reads a field).  A caller
// compiled against the first layout of version 1 (which ended with gh3) passes a SHORTER block: it is accepted and the fields it does not have
// (phi_packed, gl_nodes01, gl_weights01, eps) read as zero — the point of carrying struct_size.  A block longer than this library knows, another
// version, or one cut inside the original fields is refused.
template <class Args> static inline bool ar_args_norm(const Args* p, Args* out) {
  if (!p || p->version != 1 || p->struct_size < offsetof(Args, phi_packed) || p->struct_size > sizeof(Args)) return false;
  std::memset(out, 0, sizeof(*out));
  std::memcpy(out, p, p->struct_size);
  out->struct_size = sizeof(Args);
  return true;
}

}  // namespace zk
