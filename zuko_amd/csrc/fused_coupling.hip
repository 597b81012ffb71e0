// zuko_amd — fused COUPLING transform: dense conditioner MLP + affine map + log|det J| in one launch.
//
// Replaces, for one GeneralCouplingTransform of NICE / RealNVP (zuko/flows/coupling.py:128-136 `meta`,
// zuko/transforms.py:1040-1048 / :1068-1073 `CouplingTransform`):
//     x_a, x_b = split(x);  phi = MLP(cat(x_a, c))  (zuko/nn.py:13-15 per layer + activations);
//     y_b, ladj = MonotonicAffineTransform(*unpack(phi)).call_and_ladj(x_b)  (zuko/transforms.py:436-446);  y = merge(x_a, y_b)
// Layer by layer this moves every hidden activation through HBM ([N, 512] fp32 = 1 GiB per layer at cfg4's 2^19 rows per
// GPU); here a wavefront carries 16 samples through all layers with the activations in registers, exactly as the
// autoregressive kernel (fused_ar.hip) does, but for hidden widths up to 512:
//   * every layer is computed transposed, H^T = W X^T, on v_mfma_f32_16x16x4_f32 (exact fp32); the D fragment of a layer
//     is the B operand of the next one, so nothing is shuffled or staged between layers;
//   * 32 + 32 activation tiles = 256 VGPRs/AGPRs: one wavefront per SIMD (launch_bounds(256, 1)), four wavefronts = 64
//     samples per workgroup share the weight stream (2.9 MB per transform at cfg4, L2-resident) through a 3 x 24 KiB LDS
//     ring filled by global_load_lds two chunks ahead;
//   * the split / merge of CouplingTransform is index arithmetic on a wave-private LDS image of the 16 input rows: the
//     conditioner's B operands are gathered from it (idx_a), the affine map overwrites the moved columns (idx_b) in
//     place, and the image leaves as whole rows.
// Host-side planning (stream order, bias image, index maps): zuko_amd/coupling_plan.py.
#include "../../include/zuko_amd.h"
#include "fused_ar_half_impl.h"  // what the autoregressive kernels already have: ArRingS, ars_for, ArLane, the raw LDS reads, arx_split, arh_scale, the vector types

namespace zk {

#define CP_T 32      /* activation tiles (hidden width <= 512) */
#define CP_IT 16     /* input tiles (conditioner inputs <= 256) */
#define CP_CH 24     /* images per ring chunk: the f32 kernels and the three-part (bf16) one */
#define CPH_CH 16    /* images per ring chunk of the two-part (f16) kernel */
#define CP_NR 3
#define CP_WAVES 4
#define CP_MAXL 8

struct CpArgs {
  int64_t N;
  int D, C;                     // features of x, context width
  const float* x; int64_t ldx;
  const float* ctx; int64_t ldc;
  float* y; int64_t ldy;
  float* ladj; int accumulate;
  const float* stream;
  const float* bias;
  const int32_t* amap;          // [nit * 16]: column of x (>= 0), -(2 + c) for context column c, -1 for padding
  const int32_t* fmap;          // [NG * 8]: column of x the slot's feature lives in, -1 = padding
  int L;                        // linear layers (>= 2)
  int nit;                      // input tiles of the first layer
  int wt[CP_MAXL];              // output tiles of every hidden layer
  int width[CP_MAXL];           // hidden widths (units beyond are padding)
  int NG;                       // groups of 8 moved features
  int n_chunks, act, bias_floats;
  int bias_off[CP_MAXL];
  int xs;                       // LDS row stride (floats) of the wave-private row image
  int vec4;                     // rows of y can be written 16 bytes per lane
  int vec4_in;                  // rows of x / context can be fetched 16 bytes per lane
  int inverse;                  // x holds y: the moved half is mapped back (x_b = (y_b - shift) exp(-scale)); ladj stays that of the forward map
  float ls;
  int64_t n_tiles;
  float wdescale[CP_MAXL];      // two-part (f16) kernel: 2^-ew of every linear layer, the power of two its weights were stored with
};

// act_f32 as ONE out-of-line copy: inlined into the 128 values of cp_activate's unrolled tile loop it would not fit the instruction cache
__device__ __attribute__((noinline)) float cp_act_slow(float v, int act) { return act_f32(v, act); }

struct CpRing {
  float* lds;
  const float* stream;
  int n_chunks, pos, slot, load_chunk, load_slot, wave, lane;
  // each wave copies CP_CH / CP_WAVES consecutive tiles: one address and one M0 value per four of them, the tile selected by
  // the instruction's immediate offset (scripts/probes/dma_issue_probe.hip: ~40 cycles of issue per vector-memory
  // instruction, ~20 more per M0 write)
  template <int I> __device__ __forceinline__ void dma(const float* g, float* l) {
    if constexpr (I < CP_CH / CP_WAVES) {
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, (I - 4) * 1024, 0);
      dma<I + 1>(g, l);
    }
  }
  __device__ __forceinline__ void issue() {
    static_assert(CP_CH / CP_WAVES == 6, "immediates -4096 .. +1024 around the wave's fifth tile reach six tiles");
    const int b4 = wave * (CP_CH / CP_WAVES) + 4;
    dma<0>(stream + ((size_t)load_chunk * CP_CH + b4) * 256 + lane * 4, lds + (load_slot * CP_CH + b4) * 256);
    load_chunk = (load_chunk + 1 == n_chunks) ? 0 : load_chunk + 1;
    load_slot = (load_slot + 1 == CP_NR) ? 0 : load_slot + 1;
  }
  __device__ __forceinline__ void advance() {  // all wavefronts reach this at the same points of the (uniform) control flow
    // the oldest chunk in flight is the one about to be read: the younger (CP_NR - 2) chunks' DMAs may stay outstanding
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((CP_NR - 2) * (CP_CH / CP_WAVES)) : "memory");
    __builtin_amdgcn_s_barrier();  // bare barrier: __syncthreads() would prepend s_waitcnt vmcnt(0) and drain the look-ahead DMAs
    asm volatile("" ::: "memory");
    issue();
    slot = (slot + 1 == CP_NR) ? 0 : slot + 1;
    pos = 0;
  }
  template <int G> __device__ __forceinline__ void begin() {
    if (pos == CP_CH) advance();
  }
  __device__ __forceinline__ f32x4 tile(int t) const { return *reinterpret_cast<const f32x4*>(lds + (slot * CP_CH + pos + t) * 256 + lane * 4); }
  template <int G> __device__ __forceinline__ void commit() { pos += G; }
  __device__ __forceinline__ void end_layer() {
    if (pos != 0) pos = CP_CH;
  }
};

// the affine map of one moved feature (zuko/transforms.py:412-446), forward or inverse; l = log|dy/dx| of the FORWARD map either way
__device__ __forceinline__ void cp_affine(const CpArgs& a, float shift, float scale, float v, float& out, float& l) {
  const float lsc = softclip<float, MathFast>(scale, a.ls);
  out = a.inverse ? MathFast::div_safe(v - shift, MathFast::exp(lsc)) : v * MathFast::exp(lsc) + shift;
  l = lsc;
}

// The wave's 16 rows [x | context] -> its LDS image, by LDS-DMA (4 bytes per lane, consecutive lanes = consecutive columns of
// one row): all row pieces are in flight together and are waited for once.  (A load-to-register / ds_write loop pays one
// memory round trip per piece, each queued behind the ring DMAs in flight: measured ~20 % of the pass at D = 256.)
__device__ __forceinline__ void cp_stage_rows(const CpArgs& a, float* xw, int xs, int64_t n0, int lane) {
  const int DC = a.D + a.C;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the previous pass's reads of the image have returned
  if (a.vec4_in) {  // 16 bytes per lane: a row of 256 columns is one DMA
#pragma unroll 1
  for (int r = 0; r < 16; ++r) {
      const int64_t nr = (n0 + r < a.N) ? n0 + r : a.N - 1;
      const float* xg = a.x + nr * a.ldx;
      const float* cg = a.C ? a.ctx + nr * a.ldc - a.D : xg;
#pragma unroll 1
      for (int c0 = 0; c0 < DC; c0 += 256) {
        const int c = c0 + lane * 4;
        if (c < DC) {
          const float* g = (c < a.D ? xg : cg) + c;
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)(xw + r * xs + c0), 16, 0, 0);
        }
      }
    }
  } else
#pragma unroll 1
  for (int r = 0; r < 16; ++r) {
    const int64_t nr = (n0 + r < a.N) ? n0 + r : a.N - 1;
    const float* xg = a.x + nr * a.ldx;
    const float* cg = a.C ? a.ctx + nr * a.ldc - a.D : xg;
#pragma unroll 1
    for (int c0 = 0; c0 < DC; c0 += 64) {
      const int c = c0 + lane;
      if (c < DC) {
        const float* g = (c < a.D ? xg : cg) + c;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)(xw + r * xs + c0), 4, 0, 0);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// Results: whole rows out of the image (16 bytes per lane when the row layout allows it).
__device__ __forceinline__ void cp_store_rows(const CpArgs& a, const float* xw, int xs, int64_t n0, int lane) {
  if (a.vec4) {
#pragma unroll 1
  for (int r = 0; r < 16; ++r) {
      if (n0 + r < a.N)
#pragma unroll 1
        for (int c = lane * 4; c < a.D; c += 256) *reinterpret_cast<f32x4*>(a.y + (n0 + r) * a.ldy + c) = *reinterpret_cast<const f32x4*>(xw + r * xs + c);
    }
  } else {
#pragma unroll 1
  for (int r = 0; r < 16; ++r) {
      if (n0 + r < a.N)
#pragma unroll 1
        for (int c = lane; c < a.D; c += 64) a.y[(n0 + r) * a.ldy + c] = xw[r * xs + c];
    }
  }
}

extern __shared__ __attribute__((aligned(16))) float cp_lds[];

// ---- the frame: everything of a coupling kernel that is not its matrix part -------------------------------------------------
// LDS:  ring (CP_NR chunks) | bias image | amap (CP_IT * 16) | fmap (NG * 8) | layer words (3 * CP_MAXL: tiles, widths, bias offsets) | wave-private
// row images (16 rows x xs floats per wavefront).  ONE definition for the kernels (the carved pointers) and for cp_launch (the size).
struct CpLds {
  float* bias;
  int *amap, *fmap, *lay;
  float* rows;  // this wavefront's image
  static constexpr int bytes(int chunk, int bias_floats, int n_groups, int xs) {
    return (CP_NR * chunk * 256 + bias_floats + CP_IT * 16 + n_groups * 8 + 3 * CP_MAXL + CP_WAVES * 16 * xs) * (int)sizeof(float);
  }
  __device__ __forceinline__ CpLds(const CpArgs& a, int chunk, int wave)
      : bias(cp_lds + CP_NR * chunk * 256), amap(reinterpret_cast<int*>(bias + a.bias_floats)), fmap(amap + CP_IT * 16), lay(fmap + a.NG * 8),
        rows(reinterpret_cast<float*>(lay + 3 * CP_MAXL) + (size_t)wave * 16 * a.xs) {}
  // Cooperative copy of the launch's tables (the caller's ring start-up and workgroup barrier follow).  Per-layer scalars are read through LDS:
  // indexing the by-value kernel argument arrays with a run-time layer index would make the compiler spill the whole argument block to scratch
  // memory.  SHAPES: tiles and widths too (the generic kernel; the static-shape kernels have them as template parameters).
  template <bool SHAPES> __device__ __forceinline__ void stage(const CpArgs& a, int tid, int nit) const {
    if (tid == 0) {
#pragma unroll
      for (int l = 0; l < CP_MAXL; ++l) {
        if constexpr (SHAPES) { lay[l] = a.wt[l]; lay[CP_MAXL + l] = a.width[l]; }
        lay[2 * CP_MAXL + l] = a.bias_off[l];
      }
    }
    for (int i = tid; i < a.bias_floats; i += 256) bias[i] = a.bias[i];
    for (int i = tid; i < nit * 16; i += 256) amap[i] = a.amap[i];
    for (int i = tid; i < a.NG * 8; i += 256) fmap[i] = a.fmap[i];
  }
  __device__ __forceinline__ int tiles_of(int l) const { return __builtin_amdgcn_readfirstlane(lay[l]); }
  __device__ __forceinline__ int width_of(int l) const { return __builtin_amdgcn_readfirstlane(lay[CP_MAXL + l]); }
  __device__ __forceinline__ const float* bias_of(int l, int q) const { return bias + __builtin_amdgcn_readfirstlane(lay[2 * CP_MAXL + l]) + 4 * q; }  // this lane's units of layer l
};

// B operand values of input tile `it` of the first layer: lane (j, q) gathers units 4 q .. 4 q + 3 from its row of the image through amap
__device__ __forceinline__ f32x4 cp_gather_inputs(const CpArgs& a, const int* amap_lds, const float* xrow, int it, int q) {
  f32x4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int src = amap_lds[it * 16 + 4 * q + r];
    v[r] = src >= 0 ? xrow[src] : (src <= -2 ? xrow[a.D + (-2 - src)] : 0.f);
  }
  return v;
}

// A group of 8 moved features: lane (j, q) owns slots 2 q and 2 q + 1.  Their columns and input values are requested before the group's matrix
// instructions; cp_group_epilogue applies the two affine maps to p = (shift, scale) of slot 2 q, then of slot 2 q + 1, writes the results back
// into the row image and adds the log-derivatives to lacc.
struct CpSlots {
  int f0, f1;
  float x0, x1;
  __device__ __forceinline__ CpSlots(const int* fmap_lds, const float* xrow, int g, int q)
      : f0(fmap_lds[g * 8 + 2 * q]), f1(fmap_lds[g * 8 + 2 * q + 1]), x0(xrow[f0 < 0 ? 0 : f0]), x1(xrow[f1 < 0 ? 0 : f1]) {}
};
__device__ __forceinline__ void cp_group_epilogue(const CpArgs& a, const CpSlots& s, const f32x4& p, float* xrow, float& lacc) {
  float y0, y1, l0, l1;
  cp_affine(a, p[0], p[1], s.x0, y0, l0);
  cp_affine(a, p[2], p[3], s.x1, y1, l1);
  if (s.f0 >= 0) { xrow[s.f0] = y0; lacc += l0; }
  if (s.f1 >= 0) { xrow[s.f1] = y1; lacc += l1; }
}

// End of a pass: the wave's image leaves as whole rows, the sample's log-derivative is summed over q (two shuffles) and stored
__device__ __forceinline__ void cp_finish_rows(const CpArgs& a, const float* xw, int64_t n0, const ArLane& ln, float lacc) {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  cp_store_rows(a, xw, a.xs, n0, ln.lane);
  if (a.ladj) {
    const int64_t n = n0 + ln.j;
    lacc += __shfl_xor(lacc, 16, 64);
    lacc += __shfl_xor(lacc, 32, 64);
    if (n < a.N && ln.q == 0) a.ladj[n] = a.accumulate ? a.ladj[n] + lacc : lacc;
  }
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// The static-shape kernels read their weight images (and the split kernels their bias tiles) RAW: ArRingS::read, arx_lds_raw.  cp_settle<N> makes
// such values usable: it waits until at most N younger LDS operations are outstanding and is the only consumer of the raw registers
// (tests/test_codegen.py checks the ISA).  One overload per register set of a step: the images, or the images and the four bias tiles of an out-group.
#define CP_S4(a) "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3])
#define CP_S6(a) CP_S4(a), "+v"(a[4]), "+v"(a[5])
#define CP_S8(a) CP_S6(a), "+v"(a[6]), "+v"(a[7])
#define CP_S12(a) CP_S8(a), "+v"(a[8]), "+v"(a[9]), "+v"(a[10]), "+v"(a[11])
#define CP_SO "+v"(o0), "+v"(o1), "+v"(o2), "+v"(o3)
template <int N> __device__ __forceinline__ void cp_settle(f32x4 (&a)[4]) { asm volatile("s_waitcnt lgkmcnt(%4)" : CP_S4(a) : "n"(N)); }
template <int N> __device__ __forceinline__ void cp_settle(f32x4 (&a)[6]) { asm volatile("s_waitcnt lgkmcnt(%6)" : CP_S6(a) : "n"(N)); }
template <int N> __device__ __forceinline__ void cp_settle(f32x4 (&a)[8]) { asm volatile("s_waitcnt lgkmcnt(%8)" : CP_S8(a) : "n"(N)); }
template <int N> __device__ __forceinline__ void cp_settle(f32x4 (&a)[12]) { asm volatile("s_waitcnt lgkmcnt(%12)" : CP_S12(a) : "n"(N)); }
template <int N> __device__ __forceinline__ void cp_settle(f32x4 (&a)[8], f32x4& o0, f32x4& o1, f32x4& o2, f32x4& o3) { asm volatile("s_waitcnt lgkmcnt(%12)" : CP_S8(a), CP_SO : "n"(N)); }
template <int N> __device__ __forceinline__ void cp_settle(f32x4 (&a)[12], f32x4& o0, f32x4& o1, f32x4& o2, f32x4& o3) { asm volatile("s_waitcnt lgkmcnt(%16)" : CP_S12(a), CP_SO : "n"(N)); }

// 32 activation tiles as TWO arrays of 16: a single 512-byte array is not promoted to registers by the compiler (it stays in
// scratch memory — measured 4x slower), two 256-byte ones are.  `t` is a compile-time constant at every use after unrolling.
struct CpAct {
  f32x4 (&lo)[16];
  f32x4 (&hi)[16];
  __device__ __forceinline__ f32x4& operator[](int t) const { return t < 16 ? lo[t & 15] : hi[t & 15]; }
};

// one dense layer: out[ot] = bias + sum_it W[ot, it] in[it]; NIN = static bound of the input tiles
template <int NIN> __device__ __forceinline__ void cp_layer(CpRing& ring, int n_in, int n_out, const float* bias_q, const CpAct& in, const CpAct& out) {
#pragma unroll
  for (int otg = 0; otg < CP_T / 4; ++otg) {
    if (otg * 4 < n_out) {
#pragma unroll
      for (int t = 0; t < 4; ++t) out[otg * 4 + t] = *reinterpret_cast<const f32x4*>(bias_q + (otg * 4 + t) * 16);
#pragma unroll
      for (int it = 0; it < NIN; ++it) {
        if (it < n_in) {
          ring.template begin<4>();
          f32x4 a[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) a[t] = ring.tile(t);
          ring.template commit<4>();
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < 4; ++t) out[otg * 4 + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][r], in[it][r], out[otg * 4 + t], 0, 0, 0);
        }
      }
    }
  }
  ring.end_layer();
}

__device__ __forceinline__ void cp_activate(const CpAct& h, int n_out, int width, int act, int q) {
#pragma unroll
  for (int t = 0; t < CP_T; ++t) {
    if (t < n_out) {
      if (act == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) h[t][r] = h[t][r] < 0.f ? 0.f : h[t][r];  // NaN stays NaN, as torch.relu
      } else if (act != 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) h[t][r] = cp_act_slow(h[t][r], act);
      }
      // units beyond the layer's width are padding: keep them at exactly 0 (0 * non-finite would poison the next layer)
      if ((t + 1) * 16 > width) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (t * 16 + 4 * q + r >= width) h[t][r] = 0.f;
      }
    }
  }
}

// (Of the frame this kernel takes CpSlots / cp_group_epilogue and, on the host, CpLds::bytes.  Its LDS carve and staging, its first-layer gather and
//  its pass tail stay written out: at 512 registers with spills each of CpLds, cp_gather_inputs and cp_finish_rows moved its instruction census —
//  64 LDS reads for the first two, one vector instruction for the third; profiles/coupling_frame/census.md.)
__global__ __launch_bounds__(256, 1) void coupling_kernel(CpArgs a) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int jl = lane & 15, q = lane >> 4;

  float* bias_lds = cp_lds + CP_NR * CP_CH * 256;
  int* amap_lds = reinterpret_cast<int*>(bias_lds + a.bias_floats);
  int* fmap_lds = amap_lds + CP_IT * 16;
  float* xw = reinterpret_cast<float*>(fmap_lds + a.NG * 8 + 3 * CP_MAXL) + (size_t)wave * 16 * a.xs;
  // per-layer scalars are read through LDS: indexing the by-value kernel argument arrays with a run-time layer index
  // would make the compiler spill the whole argument block to scratch memory
  int* lay_lds = fmap_lds + a.NG * 8;  // [3 * CP_MAXL]: tiles, widths, bias offsets
  if (tid == 0) {
#pragma unroll
    for (int l = 0; l < CP_MAXL; ++l) { lay_lds[l] = a.wt[l]; lay_lds[CP_MAXL + l] = a.width[l]; lay_lds[2 * CP_MAXL + l] = a.bias_off[l]; }
  }
  for (int i = tid; i < a.bias_floats; i += 256) bias_lds[i] = a.bias[i];
  for (int i = tid; i < a.nit * 16; i += 256) amap_lds[i] = a.amap[i];
  for (int i = tid; i < a.NG * 8; i += 256) fmap_lds[i] = a.fmap[i];

  CpRing ring;
  ring.lds = cp_lds; ring.stream = a.stream; ring.n_chunks = a.n_chunks; ring.wave = wave; ring.lane = lane;
  ring.load_chunk = 0; ring.load_slot = 0;
#pragma unroll
  for (int i = 0; i < CP_NR - 1; ++i) ring.issue();
  ring.slot = CP_NR - 1;
  ring.pos = CP_CH;
  __syncthreads();

  const int xs = a.xs;
  float* xrow = xw + jl * xs;
  const int DC = a.D + a.C;

  for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const int64_t n0 = tile * 64 + wave * 16;
    const int64_t n = n0 + jl;
    const bool live = n < a.N;

    // ---- the wave's 16 rows [x | context] -> LDS image (coalesced: a row is read by consecutive lanes) ------------
    cp_stage_rows(a, xw, xs, n0, lane);

    // ---- first layer: B operands gathered from the image through idx_a ---------------------------------------------
    f32x4 out_lo[16], out_hi[16], in_lo[16], in_hi[16];
    const CpAct out{out_lo, out_hi}, in{in_lo, in_hi};
#pragma unroll
    for (int it = 0; it < CP_T; ++it) in[it] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < CP_IT; ++it) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (it < a.nit) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int src = amap_lds[it * 16 + 4 * q + r];
          v[r] = src >= 0 ? xrow[src] : (src <= -2 ? xrow[a.D + (-2 - src)] : 0.f);
        }
      }
      in[it] = v;
    }
    int n_prev = __builtin_amdgcn_readfirstlane(lay_lds[0]);
    cp_layer<CP_IT>(ring, a.nit, n_prev, bias_lds + __builtin_amdgcn_readfirstlane(lay_lds[2 * CP_MAXL]) + 4 * q, in, out);
    cp_activate(out, n_prev, __builtin_amdgcn_readfirstlane(lay_lds[CP_MAXL]), a.act, q);
    // ---- further hidden layers --------------------------------------------------------------------------------------
    for (int l = 1; l < a.L - 1; ++l) {
#pragma unroll
      for (int t = 0; t < CP_T; ++t) in[t] = out[t];
      const int n_out = __builtin_amdgcn_readfirstlane(lay_lds[l]);
      cp_layer<CP_T>(ring, n_prev, n_out, bias_lds + __builtin_amdgcn_readfirstlane(lay_lds[2 * CP_MAXL + l]) + 4 * q, in, out);
      cp_activate(out, n_out, __builtin_amdgcn_readfirstlane(lay_lds[CP_MAXL + l]), a.act, q);
      n_prev = n_out;
    }
    // ---- last layer + affine map, one group of 8 moved features at a time (lane (j, q): slots 2 q, 2 q + 1) -------
    const int n_last_in = n_prev;
    const float* bias_last = bias_lds + __builtin_amdgcn_readfirstlane(lay_lds[2 * CP_MAXL + a.L - 1]) + 4 * q;
    float lacc = 0.f;
    for (int g = 0; g < a.NG; ++g) {
      const CpSlots slots(fmap_lds, xrow, g, q);
      f32x4 acc0 = *reinterpret_cast<const f32x4*>(bias_last + g * 16), acc1 = {0.f, 0.f, 0.f, 0.f};  // two chains: a dependent one would wait 40 cycles per MFMA
#pragma unroll
      for (int it = 0; it < CP_T; it += 2) {
        if (it < n_last_in) {
          ring.template begin<1>();
          const f32x4 w0 = ring.tile(0);
          ring.template commit<1>();
#pragma unroll
          for (int r = 0; r < 4; ++r) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[r], out[it][r], acc0, 0, 0, 0);
        }
        if (it + 1 < n_last_in) {
          ring.template begin<1>();
          const f32x4 w1 = ring.tile(0);
          ring.template commit<1>();
#pragma unroll
          for (int r = 0; r < 4; ++r) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[r], out[it + 1][r], acc1, 0, 0, 0);
        }
      }
      cp_group_epilogue(a, slots, acc0 + acc1, xrow, lacc);
    }
    ring.end_layer();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    // ---- results: whole rows out of the image -------------------------------------------------------------------------
    cp_store_rows(a, xw, xs, n0, lane);
    if (a.ladj) {
      lacc += __shfl_xor(lacc, 16, 64);
      lacc += __shfl_xor(lacc, 32, 64);
      if (live && q == 0) a.ladj[n] = a.accumulate ? a.ladj[n] + lacc : lacc;
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // look-ahead DMAs must land before the LDS is released
}


// ---- static-shape fast path ----------------------------------------------------------------------------------------------
// Same data flow, with the layer shapes as template parameters (NIT input tiles, every hidden layer HT tiles wide, NG
// groups): no per-tile guards, and the position of every weight tile inside the pass is a compile-time constant, so the ring
// refill (barrier + DMA issue) is emitted only where that position is a multiple of the chunk size and the code between
// two refills is one basic block the scheduler can software-pipeline (ds_read of the next tiles above the current MFMAs).
// The ring is the autoregressive static-shape kernels' (fused_ar_static_impl.h): raw reads at static positions, refills where a position is a
// multiple of the chunk size; its ablation switches (ARX_ABL 1: no DMAs, 4: no barrier) serve probe builds of these kernels too.
typedef ArRingS<CP_WAVES, CP_CH, CP_NR> CpRingS;   // coupling_kernel_static, coupling_kernel_split
typedef ArRingS<CP_WAVES, CPH_CH, CP_NR> CpRingH;  // coupling_kernel_half

template <int NIN, int HT> __device__ __forceinline__ void cp_layer_static(CpRingS& ring, const float* bias_q, const CpAct& in, const CpAct& out) {
  // software pipeline: the four A tiles of step s + 1 are requested (into the other register set) before the 16 MFMAs of
  // step s are issued, so the LDS round trip hides behind 512 cycles of matrix work (one wavefront per SIMD: there is no
  // partner wave to hide it)
  constexpr int STEPS = (HT / 4) * NIN;
  f32x4 a[2][4];
  ars_for<4>([&](auto t) ARS_ALWAYS_INLINE { a[0][t] = ring.template read<decltype(t)::value>(); });
  ars_for<STEPS>([&](auto st_) ARS_ALWAYS_INLINE {
    constexpr int st = st_, otg = st / NIN, it = st % NIN;
    if constexpr (it == 0) {
      ars_for<4>([&](auto t) ARS_ALWAYS_INLINE { out[otg * 4 + t] = *reinterpret_cast<const f32x4*>(bias_q + (otg * 4 + t) * 16); });
    }
    if constexpr (st + 1 < STEPS) {
      ars_for<4>([&](auto t) ARS_ALWAYS_INLINE { a[(st + 1) & 1][t] = ring.template read<(st + 1) * 4 + decltype(t)::value>(); });
      cp_settle<4>(a[st & 1]);
    } else {
      cp_settle<0>(a[st & 1]);
    }
    __builtin_amdgcn_sched_barrier(0);
    ars_for<4>([&](auto r) ARS_ALWAYS_INLINE {
      ars_for<4>([&](auto t) ARS_ALWAYS_INLINE { out[otg * 4 + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st & 1][t][(int)r], in[it][(int)r], out[otg * 4 + t], 0, 0, 0); });
    });
    __builtin_amdgcn_sched_barrier(0);
  });
}

template <int NIT, int HT> __global__ __launch_bounds__(256, 1) void coupling_kernel_static(CpArgs a) {
  static_assert(HT % 4 == 0 && HT <= CP_T && NIT <= CP_IT, "shape");
  const ArLane ln;
  const int lane = ln.lane, wave = ln.wave, q = ln.q;
  const CpLds lds(a, CP_CH, wave);
  lds.stage<false>(a, ln.tid, NIT);
  CpRingS ring;
  ring.start(cp_lds, a.stream, a.n_chunks, wave, lane);
  __syncthreads();

  float* const xw = lds.rows;
  float* const xrow = xw + ln.j * a.xs;
  for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const int64_t n0 = tile * 64 + wave * 16;
    cp_stage_rows(a, xw, a.xs, n0, lane);

    f32x4 out_lo[16], out_hi[16], in_lo[16], in_hi[16];
    const CpAct out{out_lo, out_hi}, in{in_lo, in_hi};
#pragma unroll
    for (int it = 0; it < NIT; ++it) in[it] = cp_gather_inputs(a, lds.amap, xrow, it, q);
    cp_layer_static<NIT, HT>(ring, lds.bias_of(0, q), in, out);
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[t][r] = out[t][r] < 0.f ? 0.f : out[t][r];
    for (int l = 1; l < a.L - 1; ++l) {
#pragma unroll
      for (int t = 0; t < HT; ++t) in[t] = out[t];
      cp_layer_static<HT, HT>(ring, lds.bias_of(l, q), in, out);
#pragma unroll
      for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[t][r] = out[t][r] < 0.f ? 0.f : out[t][r];
    }
    const float* bias_last = lds.bias_of(a.L - 1, q);
    float lacc = 0.f;
    // groups are walked in triples so that the tile positions are static: HT tiles per group (HT = 32: not a multiple of the chunk), 3 * HT per triple
    static_assert((3 * HT) % CP_CH == 0, "three groups of the last layer must fill whole chunks");
    for (int g3 = 0; g3 < a.NG; g3 += 3) {
      ars_for<3>([&](auto gg_) ARS_ALWAYS_INLINE {
        constexpr int gg = gg_;
        const int g = g3 + gg;
        if (g < a.NG) {
          const CpSlots slots(lds.fmap, xrow, g, q);
          // four accumulators (one per tile of the step): a dependent MFMA every fourth issue, as in the hidden layers
          f32x4 acc[4] = {*reinterpret_cast<const f32x4*>(bias_last + g * 16), {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
          f32x4 w[2][4];  // four tiles per step, the next step requested before this step's MFMAs
          ars_for<4>([&](auto t) ARS_ALWAYS_INLINE { w[0][t] = ring.template read<gg * HT + decltype(t)::value>(); });
          ars_for<HT / 4>([&](auto k_) ARS_ALWAYS_INLINE {
            constexpr int k = k_, it = 4 * k;
            if constexpr (it + 4 < HT) {
              ars_for<4>([&](auto t) ARS_ALWAYS_INLINE { w[(k + 1) & 1][t] = ring.template read<gg * HT + it + 4 + decltype(t)::value>(); });
              cp_settle<4>(w[k & 1]);
            } else {
              cp_settle<0>(w[k & 1]);
            }
            __builtin_amdgcn_sched_barrier(0);
            ars_for<4>([&](auto r) ARS_ALWAYS_INLINE {
              ars_for<4>([&](auto t) ARS_ALWAYS_INLINE { acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[k & 1][t][(int)r], out[it + t][(int)r], acc[t], 0, 0, 0); });
            });
            __builtin_amdgcn_sched_barrier(0);
          });
          cp_group_epilogue(a, slots, (acc[0] + acc[1]) + (acc[2] + acc[3]), xrow, lacc);
        }
      });
    }
    cp_finish_rows(a, xw, n0, ln, lacc);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // look-ahead DMAs must land before the LDS is released
}

// ---- operand-split twin of the static-shape path ----------------------------------------------------------------------------------
// The f32 matrix instruction bounds the kernels above (0.81 of its peak at cfg4, profiles/r03) and runs at 1/16 of the bf16 rate;
// gfx950 has no tf32.  As in csrc/fused_ar_split_impl.h every f32 operand is written as h + m + l in bf16 (exact to 2^-25) and a
// product is the six partial products down to 2^-18 on v_mfma_f32_16x16x32_bf16 with f32 accumulation: the error of an f32 dot
// product at 6/16 of the matrix time.  A stream BLOCK is the 16 x 32 weight block (out tile, PAIR of in tiles) as three 1 KiB bf16
// images; a lane's 8 values are [4 units of in tile 2 ip | the same 4 units of in tile 2 ip + 1], which is how the activations sit in
// the accumulator registers, so a layer's D fragments become the next layer's B operands by an in-register conversion.  One
// wavefront per SIMD: a step is 4 out tiles x 1 in pair (12 images, 24 matrix instructions issued term by term, so the same
// accumulator is touched every fourth instruction and never waits for its predecessor).
struct CpBv {  // B operands (h, m, l parts) of 16 activation pairs, as arrays small enough to be promoted to registers
  bf16x8 (&hlo)[8]; bf16x8 (&hhi)[8]; bf16x8 (&mlo)[8]; bf16x8 (&mhi)[8]; bf16x8 (&llo)[8]; bf16x8 (&lhi)[8];
  __device__ __forceinline__ bf16x8& h(int p) const { return p < 8 ? hlo[p & 7] : hhi[p & 7]; }
  __device__ __forceinline__ bf16x8& m(int p) const { return p < 8 ? mlo[p & 7] : mhi[p & 7]; }
  __device__ __forceinline__ bf16x8& l(int p) const { return p < 8 ? llo[p & 7] : lhi[p & 7]; }
  __device__ __forceinline__ void split(int p, const f32x4& lo, const f32x4& hi) const {  // pair p = arx_split of two activation tiles
    ArxB b;
    arx_split(lo, hi, b);
    h(p) = b.h; m(p) = b.m; l(p) = b.l;
  }
};

// one dense layer: out[ot] = bias + sum_ip W[ot, ip] in[ip]; NP in pairs, HT out tiles
template <int NP, int HT> __device__ __forceinline__ void cp_layer_split(CpRingS& ring, const float* bias_q, const CpBv& in, const CpAct& out) {
  constexpr int STEPS = (HT / 4) * NP;
  f32x4 a[2][12];  // images (t, part) of the step: a[.][3 t + part], part 0 = h, 1 = m, 2 = l
  ars_for<12>([&](auto i) ARS_ALWAYS_INLINE { a[0][i] = ring.template read<decltype(i)::value>(); });
  // The out-group's accumulators start at the bias, read RAW in front of the next step's images: older than those twelve, the counted wait of the
  // step settles them too.  (As compiler-visible loads their wait was lgkmcnt(0) — the compiler cannot count the raw reads — in front of the group's
  // first matrix instruction: the twelve look-ahead images drained with it, once per out-group, with no second wavefront on the SIMD to hide it.)
  const unsigned bias_addr = arx_lds_addr(bias_q);
  ars_for<STEPS>([&](auto st_) ARS_ALWAYS_INLINE {
    constexpr int st = st_, otg = st / NP, ip = st % NP;
    if constexpr (ip == 0) {
      ars_for<4>([&](auto t) ARS_ALWAYS_INLINE { out[otg * 4 + t] = arx_lds_raw<(otg * 4 + decltype(t)::value) * 64>(bias_addr); });
    }
    if constexpr (st + 1 < STEPS) {
      ars_for<12>([&](auto i) ARS_ALWAYS_INLINE { a[(st + 1) & 1][i] = ring.template read<(st + 1) * 12 + decltype(i)::value>(); });
      if constexpr (ip == 0) cp_settle<12>(a[st & 1], out[otg * 4 + 0], out[otg * 4 + 1], out[otg * 4 + 2], out[otg * 4 + 3]);
      else cp_settle<12>(a[st & 1]);
    } else {
      if constexpr (ip == 0) cp_settle<0>(a[st & 1], out[otg * 4 + 0], out[otg * 4 + 1], out[otg * 4 + 2], out[otg * 4 + 3]);
      else cp_settle<0>(a[st & 1]);
    }
    __builtin_amdgcn_sched_barrier(0);
    const bf16x8 bh = in.h(ip), bm = in.m(ip), bl = in.l(ip);
    // six partial products, smallest first, each over the four out tiles of the step
    ars_for<4>([&](auto t) ARS_ALWAYS_INLINE { ARX_MFMA(a[st & 1][3 * t + 2], bh, out[otg * 4 + t]); });
    ars_for<4>([&](auto t) ARS_ALWAYS_INLINE { ARX_MFMA(a[st & 1][3 * t + 0], bl, out[otg * 4 + t]); });
    ars_for<4>([&](auto t) ARS_ALWAYS_INLINE { ARX_MFMA(a[st & 1][3 * t + 1], bm, out[otg * 4 + t]); });
    ars_for<4>([&](auto t) ARS_ALWAYS_INLINE { ARX_MFMA(a[st & 1][3 * t + 1], bh, out[otg * 4 + t]); });
    ars_for<4>([&](auto t) ARS_ALWAYS_INLINE { ARX_MFMA(a[st & 1][3 * t + 0], bm, out[otg * 4 + t]); });
    ars_for<4>([&](auto t) ARS_ALWAYS_INLINE { ARX_MFMA(a[st & 1][3 * t + 0], bh, out[otg * 4 + t]); });
    __builtin_amdgcn_sched_barrier(0);
  });
}

// ReLU + conversion of the HT out tiles into the next layer's B operands
template <int HT> __device__ __forceinline__ void cp_convert(const CpAct& out, const CpBv& in) {
  ars_for<HT / 2>([&](auto p_) ARS_ALWAYS_INLINE {
    constexpr int p = p_;
    f32x4 lo = out[2 * p], hi = out[2 * p + 1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      lo[r] = lo[r] < 0.f ? 0.f : lo[r];  // NaN stays NaN, as torch.relu
      hi[r] = hi[r] < 0.f ? 0.f : hi[r];
    }
    in.split(p, lo, hi);
  });
}

template <int NIT, int HT> __global__ __launch_bounds__(256, 1) void coupling_kernel_split(CpArgs a) {
  static_assert(HT % 4 == 0 && HT <= CP_T && NIT <= CP_IT && NIT % 2 == 0 && (12 * (NIT / 2) * (HT / 4)) % CP_CH == 0 && (12 * (HT / 2) * (HT / 4)) % CP_CH == 0 && (3 * (HT / 2)) % CP_CH == 0,
                "every layer and every group of the last layer fills whole chunks");
  const ArLane ln;
  const int lane = ln.lane, wave = ln.wave, q = ln.q;
  const CpLds lds(a, CP_CH, wave);
  lds.stage<false>(a, ln.tid, NIT);
  CpRingS ring;  // (start-up written out: as ArRingS::start this kernel gains 8 registers and 27 vector instructions, profiles/coupling_frame/census.md)
  ring.lds = cp_lds; ring.stream = a.stream; ring.n_chunks = a.n_chunks; ring.wave = wave; ring.lane = lane;
  ring.load_chunk = 0; ring.load_slot = 0;
#pragma unroll
  for (int i = 0; i < CP_NR - 1; ++i) ring.issue();
  ring.slot = CP_NR - 1;
  ring.lds_off = (unsigned)(size_t)((__attribute__((address_space(3))) float*)cp_lds);
  ring.cur_off = ring.lds_off;
  __syncthreads();

  float* const xw = lds.rows;
  float* const xrow = xw + ln.j * a.xs;
  for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const int64_t n0 = tile * 64 + wave * 16;
    cp_stage_rows(a, xw, a.xs, n0, lane);

    f32x4 out_lo[16], out_hi[16];
    bf16x8 bhl[8], bhh[8], bml[8], bmh[8], bll[8], blh[8];
    const CpAct out{out_lo, out_hi};
    const CpBv in{bhl, bhh, bml, bmh, bll, blh};
    // first layer: B operands gathered from the row image through idx_a, converted pair by pair
    ars_for<NIT / 2>([&](auto p_) ARS_ALWAYS_INLINE {
      constexpr int p = p_;
      const f32x4 lo = cp_gather_inputs(a, lds.amap, xrow, 2 * p, q), hi = cp_gather_inputs(a, lds.amap, xrow, 2 * p + 1, q);
      in.split(p, lo, hi);
    });
    cp_layer_split<NIT / 2, HT>(ring, lds.bias_of(0, q), in, out);
    cp_convert<HT>(out, in);
    for (int l = 1; l < a.L - 1; ++l) {
      cp_layer_split<HT / 2, HT>(ring, lds.bias_of(l, q), in, out);
      cp_convert<HT>(out, in);
    }
    // last layer + affine map: one group of 8 moved features = one out tile = HT / 2 blocks, two blocks per step on six accumulators
    const float* bias_last = lds.bias_of(a.L - 1, q);
    float lacc = 0.f;
    for (int g = 0; g < a.NG; ++g) {
      const CpSlots slots(lds.fmap, xrow, g, q);
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      f32x4 cH[2] = {*reinterpret_cast<const f32x4*>(bias_last + g * 16), zero}, cM[2] = {zero, zero}, cS[2] = {zero, zero};
      f32x4 w[2][6];  // images of the step's two blocks: w[.][3 b + part]
      constexpr int KS = HT / 4;  // steps per group
      ars_for<6>([&](auto i) ARS_ALWAYS_INLINE { w[0][i] = ring.template read<decltype(i)::value>(); });
      ars_for<KS>([&](auto k_) ARS_ALWAYS_INLINE {
        constexpr int k = k_;
        if constexpr (k + 1 < KS) {
          ars_for<6>([&](auto i) ARS_ALWAYS_INLINE { w[(k + 1) & 1][i] = ring.template read<(k + 1) * 6 + decltype(i)::value>(); });
          cp_settle<6>(w[k & 1]);
        } else {
          cp_settle<0>(w[k & 1]);
        }
        __builtin_amdgcn_sched_barrier(0);
        ars_for<2>([&](auto b) ARS_ALWAYS_INLINE { ARX_MFMA(w[k & 1][3 * b + 2], in.h(2 * k + b), cS[b]); });
        ars_for<2>([&](auto b) ARS_ALWAYS_INLINE { ARX_MFMA(w[k & 1][3 * b + 1], in.h(2 * k + b), cM[b]); });
        ars_for<2>([&](auto b) ARS_ALWAYS_INLINE { ARX_MFMA(w[k & 1][3 * b + 0], in.h(2 * k + b), cH[b]); });
        ars_for<2>([&](auto b) ARS_ALWAYS_INLINE { ARX_MFMA(w[k & 1][3 * b + 0], in.l(2 * k + b), cS[b]); });
        ars_for<2>([&](auto b) ARS_ALWAYS_INLINE { ARX_MFMA(w[k & 1][3 * b + 0], in.m(2 * k + b), cM[b]); });
        ars_for<2>([&](auto b) ARS_ALWAYS_INLINE { ARX_MFMA(w[k & 1][3 * b + 1], in.m(2 * k + b), cS[b]); });
        __builtin_amdgcn_sched_barrier(0);
      });
      arx_mfma_guard<true>(cS[1]);  // wait states behind the group's last matrix instruction: one wavefront per SIMD, accumulators may sit in AGPRs
      cp_group_epilogue(a, slots, ((cS[0] + cS[1]) + (cM[0] + cM[1])) + (cH[0] + cH[1]), xrow, lacc);
    }
    cp_finish_rows(a, xw, n0, ln, lacc);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // look-ahead DMAs must land before the LDS is released
}


// ---- TWO-PART operand split (round 6; csrc/fused_ar_half_impl.h has the arithmetic's full description) ------------------------------
// Every f32 operand as two f16 numbers after an exact power-of-two scaling (weights: per layer, host; activations: per SAMPLE and layer, from the
// largest magnitude of the sample's input vector — a lane holds one sample, two shuffles), three partial products lh + hl + hh on
// v_mfma_f32_16x16x32_f16, the accumulator back through one fma with 2^-(ew + ea) and the bias: half the matrix instructions of
// coupling_kernel_split, two 1 KiB images per 16 x 32 block (16-image chunks: every layer and every group of the last layer fills whole chunks).
// One wavefront per SIMD, more than 256 registers: the accumulators of a step are pinned to VGPRs and the step's matrix instructions are ONE
// assembly block (hipcc under-counts the wait states behind a v_mfma_f32_16x16x32_f16 whose destination is an AGPR: profiles/r06/inverse.md),
// with 12 wait states in front of the vector instructions that read them.
struct CpBh {  // B operands (h, l parts) of 16 activation pairs
  f16x8 (&hlo)[8]; f16x8 (&hhi)[8]; f16x8 (&llo)[8]; f16x8 (&lhi)[8];
  __device__ __forceinline__ f16x8& h(int p) const { return p < 8 ? hlo[p & 7] : hhi[p & 7]; }
  __device__ __forceinline__ f16x8& l(int p) const { return p < 8 ? llo[p & 7] : lhi[p & 7]; }
};
// (plain expressions: arh_split's pinned instruction pairs are another instruction sequence)
__device__ __forceinline__ void cph_split(const f32x4& lo, const f32x4& hi, float s, f16x8& h, f16x8& l) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float v = (e < 4 ? lo[e] : hi[e - 4]) * s;
    const _Float16 hh = (_Float16)v;
    h[e] = hh; l[e] = (_Float16)(v - (float)hh);
  }
}
// the twelve matrix instructions of a step (4 out tiles x 3 partial products, term by term: an accumulator is touched every fourth instruction),
// images a[2 t] = h, a[2 t + 1] = l of out tile t; FIRST: the accumulators start at zero; LAST: wait states for the vector instructions that follow
template <bool FIRST, bool LAST> __device__ __forceinline__ void cph_step(f32x4 (&acc)[4], f32x4 (&a)[8], const f16x8& bh, const f16x8& bl) {
  if constexpr (FIRST) {
    asm volatile("s_nop 1\n\t"
                 "v_mfma_f32_16x16x32_f16 %0, %5, %12, 0\n\tv_mfma_f32_16x16x32_f16 %1, %7, %12, 0\n\tv_mfma_f32_16x16x32_f16 %2, %9, %12, 0\n\tv_mfma_f32_16x16x32_f16 %3, %11, %12, 0\n\t"
                 "v_mfma_f32_16x16x32_f16 %0, %4, %13, %0\n\tv_mfma_f32_16x16x32_f16 %1, %6, %13, %1\n\tv_mfma_f32_16x16x32_f16 %2, %8, %13, %2\n\tv_mfma_f32_16x16x32_f16 %3, %10, %13, %3\n\t"
                 "v_mfma_f32_16x16x32_f16 %0, %4, %12, %0\n\tv_mfma_f32_16x16x32_f16 %1, %6, %12, %1\n\tv_mfma_f32_16x16x32_f16 %2, %8, %12, %2\n\tv_mfma_f32_16x16x32_f16 %3, %10, %12, %3"
                 : "=&v"(acc[0]), "=&v"(acc[1]), "=&v"(acc[2]), "=&v"(acc[3])
                 : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), "v"(bh), "v"(bl));
  } else {
    asm volatile("s_nop 1\n\t"
                 "v_mfma_f32_16x16x32_f16 %0, %5, %12, %0\n\tv_mfma_f32_16x16x32_f16 %1, %7, %12, %1\n\tv_mfma_f32_16x16x32_f16 %2, %9, %12, %2\n\tv_mfma_f32_16x16x32_f16 %3, %11, %12, %3\n\t"
                 "v_mfma_f32_16x16x32_f16 %0, %4, %13, %0\n\tv_mfma_f32_16x16x32_f16 %1, %6, %13, %1\n\tv_mfma_f32_16x16x32_f16 %2, %8, %13, %2\n\tv_mfma_f32_16x16x32_f16 %3, %10, %13, %3\n\t"
                 "v_mfma_f32_16x16x32_f16 %0, %4, %12, %0\n\tv_mfma_f32_16x16x32_f16 %1, %6, %12, %1\n\tv_mfma_f32_16x16x32_f16 %2, %8, %12, %2\n\tv_mfma_f32_16x16x32_f16 %3, %10, %12, %3"
                 : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3])
                 : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), "v"(bh), "v"(bl));
  }
  if constexpr (LAST) asm volatile("s_nop 11" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
}

// one dense layer: out[ot] = fma(W' in', d, bias) over (4 out tiles, 1 in pair) steps; NP in pairs, HT out tiles
template <int NP, int HT> __device__ __forceinline__ void cph_layer(CpRingH& ring, const float* bias_q, const CpBh& in, const CpAct& out, float d) {
  constexpr int STEPS = (HT / 4) * NP;
  f32x4 a[2][8];
  f32x4 acc[4], bs[4];
  ars_for<8>([&](auto i) ARS_ALWAYS_INLINE { a[0][i] = ring.template read<decltype(i)::value>(); });
  const unsigned bias_addr = arx_lds_addr(bias_q);
  ars_for<STEPS>([&](auto st_) ARS_ALWAYS_INLINE {
    constexpr int st = st_, otg = st / NP, ip = st % NP;
    constexpr bool first = ip == 0, last = ip == NP - 1;
    if constexpr (last) {  // the out-group's bias tiles: raw reads in front of the look-ahead request of the group's LAST step, whose counted wait settles them
      ars_for<4>([&](auto t) ARS_ALWAYS_INLINE { bs[t] = arx_lds_raw<(otg * 4 + decltype(t)::value) * 64>(bias_addr); });
    }
    if constexpr (st + 1 < STEPS) {
      ars_for<8>([&](auto i) ARS_ALWAYS_INLINE { a[(st + 1) & 1][i] = ring.template read<(st + 1) * 8 + decltype(i)::value>(); });
      if constexpr (last) cp_settle<8>(a[st & 1], bs[0], bs[1], bs[2], bs[3]);
      else cp_settle<8>(a[st & 1]);
    } else {
      if constexpr (last) cp_settle<0>(a[st & 1], bs[0], bs[1], bs[2], bs[3]);
      else cp_settle<0>(a[st & 1]);
    }
    __builtin_amdgcn_sched_barrier(0);
    cph_step<first, last>(acc, a[st & 1], in.h(ip), in.l(ip));
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (last) {
      ars_for<4>([&](auto t) ARS_ALWAYS_INLINE {
#pragma unroll
        for (int r = 0; r < 4; ++r) out[otg * 4 + t][r] = __builtin_fmaf(acc[t][r], d, bs[t][r]);
      });
    }
  });
}

// ReLU + per-sample scale + conversion of the HT out tiles into the next layer's B operands; returns 2^-ea
template <int HT> __device__ __forceinline__ float cph_convert(const CpAct& out, const CpBh& in) {
  float amax = 0.f;
  ars_for<HT>([&](auto t_) ARS_ALWAYS_INLINE {
    constexpr int t = t_;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      out[t][r] = out[t][r] < 0.f ? 0.f : out[t][r];  // NaN stays NaN, as torch.relu
      amax = fmaxf(amax, out[t][r]);
    }
  });
  float s, inv_s;
  arh_scale(amax, s, inv_s);
  ars_for<HT / 2>([&](auto p_) ARS_ALWAYS_INLINE {
    constexpr int p = p_;
    cph_split(out[2 * p], out[2 * p + 1], s, in.h(p), in.l(p));
  });
  return inv_s;
}

template <int NIT, int HT> __global__ __launch_bounds__(256, 1) void coupling_kernel_half(CpArgs a) {
  static_assert(HT % 4 == 0 && HT <= CP_T && NIT <= CP_IT && NIT % 2 == 0 && (8 * (NIT / 2) * (HT / 4)) % CPH_CH == 0 && (8 * (HT / 2) * (HT / 4)) % CPH_CH == 0 && (2 * (HT / 2)) % CPH_CH == 0,
                "every layer and every group of the last layer fills whole chunks");
  const ArLane ln;
  const int lane = ln.lane, wave = ln.wave, q = ln.q;
  const CpLds lds(a, CPH_CH, wave);
  lds.stage<false>(a, ln.tid, NIT);
  CpRingH ring;
  ring.start(cp_lds, a.stream, a.n_chunks, wave, lane);
  __syncthreads();

  float* const xw = lds.rows;
  float* const xrow = xw + ln.j * a.xs;
  for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const int64_t n0 = tile * 64 + wave * 16;
    cp_stage_rows(a, xw, a.xs, n0, lane);

    f32x4 out_lo[16], out_hi[16];
    f16x8 bhl[8], bhh[8], bll[8], blh[8];
    const CpAct out{out_lo, out_hi};
    const CpBh in{bhl, bhh, bll, blh};
    float inv_s;
    {  // first layer: B operands gathered from the row image through idx_a, scaled by the sample's own power of two, converted pair by pair
      f32x4 v[NIT];
      float amax = 0.f;
      ars_for<NIT>([&](auto t_) ARS_ALWAYS_INLINE {
        constexpr int t = t_;
        v[t] = cp_gather_inputs(a, lds.amap, xrow, t, q);
#pragma unroll
        for (int r = 0; r < 4; ++r) amax = fmaxf(amax, fabsf(v[t][r]));
      });
      float s;
      arh_scale(amax, s, inv_s);
      ars_for<NIT / 2>([&](auto p_) ARS_ALWAYS_INLINE { constexpr int p = p_; cph_split(v[2 * p], v[2 * p + 1], s, in.h(p), in.l(p)); });
    }
    cph_layer<NIT / 2, HT>(ring, lds.bias_of(0, q), in, out, a.wdescale[0] * inv_s);
    inv_s = cph_convert<HT>(out, in);
    for (int l = 1; l < a.L - 1; ++l) {
      cph_layer<HT / 2, HT>(ring, lds.bias_of(l, q), in, out, a.wdescale[l] * inv_s);
      inv_s = cph_convert<HT>(out, in);
    }
    // last layer + affine map: one group of 8 moved features = one out tile = HT / 2 blocks, two blocks per step on two accumulators
    const float* bias_last = lds.bias_of(a.L - 1, q);
    const float dl = a.wdescale[a.L - 1] * inv_s;
    float lacc = 0.f;
    for (int g = 0; g < a.NG; ++g) {
      const CpSlots slots(lds.fmap, xrow, g, q);
      const f32x4 bg = *reinterpret_cast<const f32x4*>(bias_last + g * 16);
      f32x4 c0, c1;
      f32x4 w[2][4];  // images of the step's two blocks: w[.][2 b + part]
      constexpr int KS = HT / 4;  // steps per group
      ars_for<4>([&](auto i) ARS_ALWAYS_INLINE { w[0][i] = ring.template read<decltype(i)::value>(); });
      ars_for<KS>([&](auto k_) ARS_ALWAYS_INLINE {
        constexpr int k = k_;
        if constexpr (k + 1 < KS) {
          ars_for<4>([&](auto i) ARS_ALWAYS_INLINE { w[(k + 1) & 1][i] = ring.template read<(k + 1) * 4 + decltype(i)::value>(); });
          cp_settle<4>(w[k & 1]);
        } else {
          cp_settle<0>(w[k & 1]);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (k == 0) {
          asm volatile("s_nop 1\n\t"
                       "v_mfma_f32_16x16x32_f16 %0, %3, %6, 0\n\tv_mfma_f32_16x16x32_f16 %1, %5, %8, 0\n\t"
                       "v_mfma_f32_16x16x32_f16 %0, %2, %7, %0\n\tv_mfma_f32_16x16x32_f16 %1, %4, %9, %1\n\t"
                       "v_mfma_f32_16x16x32_f16 %0, %2, %6, %0\n\tv_mfma_f32_16x16x32_f16 %1, %4, %8, %1"
                       : "=&v"(c0), "=&v"(c1)
                       : "v"(w[0][0]), "v"(w[0][1]), "v"(w[0][2]), "v"(w[0][3]), "v"(in.h(0)), "v"(in.l(0)), "v"(in.h(1)), "v"(in.l(1)));
        } else {
          asm volatile("s_nop 1\n\t"
                       "v_mfma_f32_16x16x32_f16 %0, %3, %6, %0\n\tv_mfma_f32_16x16x32_f16 %1, %5, %8, %1\n\t"
                       "v_mfma_f32_16x16x32_f16 %0, %2, %7, %0\n\tv_mfma_f32_16x16x32_f16 %1, %4, %9, %1\n\t"
                       "v_mfma_f32_16x16x32_f16 %0, %2, %6, %0\n\tv_mfma_f32_16x16x32_f16 %1, %4, %8, %1"
                       : "+v"(c0), "+v"(c1)
                       : "v"(w[k & 1][0]), "v"(w[k & 1][1]), "v"(w[k & 1][2]), "v"(w[k & 1][3]), "v"(in.h(2 * k)), "v"(in.l(2 * k)), "v"(in.h(2 * k + 1)), "v"(in.l(2 * k + 1)));
        }
        __builtin_amdgcn_sched_barrier(0);
      });
      asm volatile("s_nop 11" : "+v"(c0), "+v"(c1));
      f32x4 p;
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] = __builtin_fmaf(c0[r] + c1[r], dl, bg[r]);  // (shift, scale) of slot 2 q, then of slot 2 q + 1
      cp_group_epilogue(a, slots, p, xrow, lacc);
    }
    cp_finish_rows(a, xw, n0, ln, lacc);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // look-ahead DMAs must land before the LDS is released
}


// ---- SPLINE twin of the generic kernel: the univariate map is the K-bin rational-quadratic spline (zuko/transforms.py:449-548) -------------------
// The coupling form of neural spline flows: NICE(..., univariate=MonotonicRQSTransform, shapes=[(K,), (K,), (K - 1,)]).  Same data flow as
// coupling_kernel up to the last hidden layer.  The last layer runs one group of FOUR moved features at a time: lane (j, q) owns slot 4 g + q of
// sample j and accumulates that slot's TOTAL = 3 K - 1 parameters in NT = ceil(TOTAL / 4) accumulators — the plan orders the weight rows so that row
// 4 q + r of out-tile t is parameter 4 t + r of slot 4 g + q (coupling_plan.py: last_rows with total = 3 K - 1), which is where the matrix instruction
// leaves it, as in the autoregressive kernels.  The stream of a group is in-tile by in-tile, the NT out-tiles of one in-tile side by side: NT
// independent accumulator chains.  rqs_lean then runs on the registers, forward or (a.inverse) inverse with the forward map's log-derivative at the
// solution.  Non-finite inputs: the conditioner is dense, so a NaN / inf among its inputs reaches every parameter through the matrix instruction
// itself (no skipped tiles, hence no flag as in ar_poison_of); all-NaN parameters give the reference's output (zk_ar_common.h: UniRqs::poison).
// cp_activate with the padding test turned round: `4 q + r >= width - 16 t` has a wave-uniform right-hand side, so the loop-invariant part is the lane's
// four unit offsets.  (Written as t * 16 + 4 * q + r >= width the compiler hoists all 128 left-hand sides out of the pass loop and keeps them in
// registers for the whole kernel: beside 32 + 32 activation tiles they do not fit, and they were this kernel's scratch.)
__device__ __forceinline__ void cp_activate_rqs(const CpAct& h, int n_out, int width, int act, int q) {
#pragma unroll
  for (int t = 0; t < CP_T; ++t) {
    if (t < n_out) {
      if (act == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) h[t][r] = h[t][r] < 0.f ? 0.f : h[t][r];  // NaN stays NaN, as torch.relu
      } else if (act != 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) h[t][r] = cp_act_slow(h[t][r], act);
      }
      // units beyond the layer's width are padding: keep them at exactly 0 (0 * non-finite would poison the next layer)
      const int left = width - t * 16;  // units of this tile that exist
      if (left < 16) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * q + r >= left) h[t][r] = 0.f;
      }
    }
  }
}

template <int K> __global__ __launch_bounds__(256, 1) void coupling_rqs_kernel(CpArgs a, RqsLeanConst lc) {
  typedef UniRqs<K, false> Uni;
  constexpr int NT = Uni::NT;
  constexpr int STEP = NT < 6 ? NT : 6;  // out-tiles read from the ring at a time: 3 / 6 / 6 of NT = 3 / 6 / 12
  static_assert(NT % STEP == 0 && CP_CH % STEP == 0, "a step never straddles two chunks");
  const ArLane ln;
  const int lane = ln.lane, wave = ln.wave, q = ln.q;
  const CpLds lds(a, CP_CH, wave);  // (fmap: 4 slots per group used of the 8 the carve reserves)
  if (ln.tid == 0) {
#pragma unroll
    for (int l = 0; l < CP_MAXL; ++l) { lds.lay[l] = a.wt[l]; lds.lay[CP_MAXL + l] = a.width[l]; lds.lay[2 * CP_MAXL + l] = a.bias_off[l]; }
  }
  for (int i = ln.tid; i < a.bias_floats; i += 256) lds.bias[i] = a.bias[i];
  for (int i = ln.tid; i < a.nit * 16; i += 256) lds.amap[i] = a.amap[i];
  for (int i = ln.tid; i < a.NG * 4; i += 256) lds.fmap[i] = a.fmap[i];

  CpRing ring;
  ring.lds = cp_lds; ring.stream = a.stream; ring.n_chunks = a.n_chunks; ring.wave = wave; ring.lane = lane;
  ring.load_chunk = 0; ring.load_slot = 0;
#pragma unroll
  for (int i = 0; i < CP_NR - 1; ++i) ring.issue();
  ring.slot = CP_NR - 1;
  ring.pos = CP_CH;
  __syncthreads();

  float* const xw = lds.rows;
  float* const xrow = xw + ln.j * a.xs;
  for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const int64_t n0 = tile * 64 + wave * 16;
    cp_stage_rows(a, xw, a.xs, n0, lane);

    f32x4 out_lo[16], out_hi[16], in_lo[16], in_hi[16];
    const CpAct out{out_lo, out_hi}, in{in_lo, in_hi};
#pragma unroll
    for (int it = 0; it < CP_T; ++it) in[it] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < CP_IT; ++it) {
      if (it < a.nit) in[it] = cp_gather_inputs(a, lds.amap, xrow, it, q);
    }
    int n_prev = lds.tiles_of(0);
    cp_layer<CP_IT>(ring, a.nit, n_prev, lds.bias_of(0, q), in, out);
    cp_activate_rqs(out, n_prev, lds.width_of(0), a.act, q);
    for (int l = 1; l < a.L - 1; ++l) {
#pragma unroll
      for (int t = 0; t < CP_T; ++t) in[t] = out[t];
      const int n_out = lds.tiles_of(l);
      cp_layer<CP_T>(ring, n_prev, n_out, lds.bias_of(l, q), in, out);
      cp_activate_rqs(out, n_out, lds.width_of(l), a.act, q);
      n_prev = n_out;
    }
    // ---- last layer + spline, one group of 4 moved features at a time (lane (j, q): slot 4 g + q) -----------------------------------------
    const float* bias_last = lds.bias_of(a.L - 1, q);
    float lacc = 0.f;
    for (int g = 0; g < a.NG; ++g) {
      const int f = lds.fmap[4 * g + q];
      const float v = xrow[f < 0 ? 0 : f];
      f32x4 acc[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = *reinterpret_cast<const f32x4*>(bias_last + (g * NT + t) * 16);
#pragma unroll
      for (int it = 0; it < CP_T; ++it) {
        if (it < n_prev) {
#pragma unroll
          for (int t0 = 0; t0 < NT; t0 += STEP) {
            ring.template begin<STEP>();
            f32x4 w[STEP];
#pragma unroll
            for (int t = 0; t < STEP; ++t) w[t] = ring.tile(t);
            ring.template commit<STEP>();
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
              for (int t = 0; t < STEP; ++t) acc[t0 + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][r], out[it][r], acc[t0 + t], 0, 0, 0);
          }
        }
      }
      // parameter p of the lane's slot = acc[p / 4][p % 4]: widths [0, K), heights [K, 2 K), derivatives [2 K, 3 K - 1)
      auto par = [&](int p) { return acc[p >> 2][p & 3]; };
      float res, lj;
      int bin;  // (unused: the three-flag form of rqs_lean returns it)
      if (a.inverse) rqs_lean<K, true, true>([&](int j) { return par(j); }, [&](int j) { return par(K + j); }, [&](int j) { return par(2 * K + j); }, lc, v, res, lj, bin);
      else rqs_lean<K, false>([&](int j) { return par(j); }, [&](int j) { return par(K + j); }, [&](int j) { return par(2 * K + j); }, lc, v, res, lj);
      if (f >= 0) { xrow[f] = res; lacc += lj; }
    }
    ring.end_layer();
    cp_finish_rows(a, xw, n0, ln, lacc);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // look-ahead DMAs must land before the LDS is released
}

}  // namespace zk

using namespace zk;

extern "C" {

// y[N, D] = merge(x_a, affine(x_b | MLP(cat(x_a, ctx)))), ladj[N] (+)= sum log|dy_b/dx_b| for one coupling transform.
// n_layers linear layers; tiles / widths: HOST arrays with the output tiles and widths of the n_layers - 1 hidden layers;
// bias_off: HOST array of n_layers offsets into the bias image; amap [nit * 16], fmap [n_groups * 8]: DEVICE index maps;
// wstream / bias: the plan of zuko_amd/coupling_plan.py.  Limits: D + C <= 1024 columns in the row image with
// 4 * 16 * (D + C + 4) * 4 bytes of LDS beside the ring (CpLds::bytes: at most 160 KiB with the 72 KiB ring of 24-image chunks), conditioner inputs <= 256, hidden widths <= 512.
static int cp_launch(int inverse, int64_t N, int D, int C, const void* x, int64_t ldx, const void* ctx, int64_t ldc, void* y, int64_t ldy, void* ladj, int accumulate,
                        const void* wstream, const void* bias, int bias_floats, const int32_t* bias_off, const int32_t* amap, int nit, const int32_t* fmap,
                        int n_groups, int n_layers, const int32_t* tiles, const int32_t* widths, int n_chunks, int act, double slope, int static_ok, void* stream,
                        const double* wdescale = nullptr, int bins = 0, double bound = 0.0) {
  if (N <= 0) return 0;
  if (n_layers < 2 || n_layers > CP_MAXL || nit < 1 || nit > CP_IT || n_groups < 1 || n_chunks < 1 || D < 2 || C < 0 || (C > 0 && !ctx)) return ZK_EINVAL;
  CpArgs a{};
  a.inverse = inverse;
  a.N = N; a.D = D; a.C = C; a.x = (const float*)x; a.ldx = ldx; a.ctx = (const float*)ctx; a.ldc = ldc; a.y = (float*)y; a.ldy = ldy;
  a.ladj = (float*)ladj; a.accumulate = accumulate; a.stream = (const float*)wstream; a.bias = (const float*)bias; a.amap = amap; a.fmap = fmap;
  a.L = n_layers; a.nit = nit; a.NG = n_groups; a.n_chunks = n_chunks; a.act = act; a.bias_floats = bias_floats;
  for (int l = 0; l < n_layers - 1; ++l) {
    if (tiles[l] < 1 || tiles[l] > CP_T) return ZK_EINVAL;
    a.wt[l] = tiles[l]; a.width[l] = widths[l];
  }
  for (int l = 0; l < n_layers; ++l) a.bias_off[l] = bias_off[l];
  a.xs = ((D + C + 3) / 4) * 4 + 4;
  a.vec4 = (D % 4 == 0) && (ldy % 4 == 0) && ((reinterpret_cast<uintptr_t>(y) & 15) == 0);
  a.vec4_in = (D % 4 == 0) && (ldx % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0) &&
              (C == 0 || ((C % 4 == 0) && (ldc % 4 == 0) && ((reinterpret_cast<uintptr_t>(ctx) & 15) == 0)));
  a.ls = (float)log(slope);
  a.n_tiles = (N + 63) / 64;
  if (CpLds::bytes(CP_CH, bias_floats, n_groups, a.xs) > 160 * 1024) return ZK_EINVAL;
  // static-shape instantiation: ReLU, every hidden layer 512 wide (32 tiles), 128 conditioner inputs (8 tiles), groups in
  // whole triples padded by the plan (cfg4 of BASELINE.json: RealNVP(256, hidden [512] * 3)); `static_ok` is the plan's word
  // that its stream has the matching layout (every layer and every triple of groups starts on a chunk boundary)
  bool same = act == 1 && nit == 8;
  for (int l = 0; l < n_layers - 1; ++l) same = same && tiles[l] == 32 && widths[l] == 512;
  const void* fn = (const void*)coupling_kernel;
  int chunk = CP_CH;
  if (static_ok == 3) {  // the plan's TWO-PART stream (coupling_plan.py: half stream): f16 images, 16-image chunks, per-layer descale factors
    if (!same || n_layers > 4 || !wdescale) return ZK_EINVAL;
    for (int l = 0; l < n_layers; ++l) {
      if (!(wdescale[l] > 0.0) || !(wdescale[l] < 1e38)) return ZK_EINVAL;
      a.wdescale[l] = (float)wdescale[l];
    }
    fn = (const void*)coupling_kernel_half<8, 32>;
    chunk = CPH_CH;
  } else if (static_ok == 2) {  // the plan's stream is the operand-split one (coupling_plan.py: split_gather): bf16 images, (4 out tiles, in pair) steps
    if (!same) return ZK_EINVAL;  // a split stream cannot be read by the f32 kernels
    fn = (const void*)coupling_kernel_split<8, 32>;
  } else if (same && static_ok) {
    fn = (const void*)coupling_kernel_static<8, 32>;
  }
  // bins != 0 (zk_coupling_*_v2 with uni_kind = 1): the spline kernel; n_groups counts groups of 4 slots, the plan's stream is the f32 one
  if (bins) {
    if (static_ok) return ZK_EINVAL;
    fn = bins == 4 ? (const void*)coupling_rqs_kernel<4> : bins == 8 ? (const void*)coupling_rqs_kernel<8> : (const void*)coupling_rqs_kernel<16>;
  }
  RqsLeanConst lc = rqs_lean_const(bound, log(slope));
  const int lds = CpLds::bytes(chunk, bias_floats, n_groups, a.xs);
  hipError_t e = grant_dyn_lds(fn, lds);
  if (e != hipSuccess) return (int)e;
  void* kargs[] = {&a, &lc};  // (lc: the spline kernels' second argument)
  e = hipLaunchKernel(fn, dim3((unsigned)(a.n_tiles < 256 ? a.n_tiles : 256)), dim3(256), kargs, lds, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  return ZK_LAUNCH_CHECK();
}


static int cp_launch_v1(int inverse, const zk_coupling_args_v1* p, void* stream) {
  if (!p || p->struct_size != sizeof(zk_coupling_args_v1) || p->version != 1) return ZK_EINVAL;
  return cp_launch(inverse, p->N, p->D, p->C, p->in, p->ldx, p->ctx, p->ldc, p->out, p->ldy, p->ladj, p->accumulate, p->wstream, p->bias, p->bias_floats, p->bias_off, p->amap,
                   p->nit, p->fmap, p->n_groups, p->n_layers, p->tiles, p->widths, p->n_chunks, p->act, p->slope, p->static_ok, stream, &p->wdescale0);
}

int zk_coupling_forward(const zk_coupling_args_v1* args, void* stream) { return cp_launch_v1(0, args, stream); }

// CouplingTransform._inverse (zuko/transforms.py:1050-1056): same launch with the affine map of the moved half inverted; ladj = the
// FORWARD map's log-determinant at the solution.
int zk_coupling_inverse(const zk_coupling_args_v1* args, void* stream) { return cp_launch_v1(1, args, stream); }

// Version 2 of the block: the v1 fields + the univariate map.  uni_kind = 0 is the v1 launch; uni_kind = 1 the K-bin spline (coupling_rqs_kernel).
// Everything is validated before the first HIP call.
static int cp_launch_v2(int inverse, const zk_coupling_args_v2* p, void* stream) {
  if (!p || p->struct_size != sizeof(zk_coupling_args_v2) || p->version != 2) return ZK_EINVAL;
  if (p->uni_kind != 0 && p->uni_kind != 1) return ZK_EINVAL;
  int bins = 0;
  if (p->uni_kind == 1) {
    if ((p->bins != 4 && p->bins != 8 && p->bins != 16) || p->static_ok != 0 || !(p->bound > 0.0) || !(p->bound < 1e30) || !(p->slope > 0.0) || !(p->slope < 1.0)) return ZK_EINVAL;
    bins = p->bins;
  }
  return cp_launch(inverse, p->N, p->D, p->C, p->in, p->ldx, p->ctx, p->ldc, p->out, p->ldy, p->ladj, p->accumulate, p->wstream, p->bias, p->bias_floats, p->bias_off, p->amap,
                   p->nit, p->fmap, p->n_groups, p->n_layers, p->tiles, p->widths, p->n_chunks, p->act, p->slope, p->static_ok, stream, &p->wdescale0, bins, p->bound);
}

int zk_coupling_forward_v2(const zk_coupling_args_v2* args, void* stream) { return cp_launch_v2(0, args, stream); }
int zk_coupling_inverse_v2(const zk_coupling_args_v2* args, void* stream) { return cp_launch_v2(1, args, stream); }

}  // extern "C"
