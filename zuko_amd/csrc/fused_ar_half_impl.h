// zuko_amd — the TWO-PART operand split of the static-shape fused autoregressive kernel (inference forward):
//
//     y, log|dy/dx| = univariate(conditioner(cat(x, c))).call_and_ladj(x)      (zuko/flows/autoregressive.py:207-218, zuko/nn.py:217-218)
//
// fused_ar_split_impl.h writes every f32 operand as three bf16 numbers and needs SIX matrix instructions per 16 x 32 weight block.  Round 6
// measured that on a SIMD whose two wavefronts keep the matrix pipe full, vector instructions add to the matrix time wherever they stand
// (profiles/r06/headline.md): the launch is matrix time + vector issue time + waits, and only FEWER instructions make it shorter.  Here an
// operand is the sum of TWO f16 numbers, h = f16(v), l = f16(v - h) (11 + 11 significant bits: |v - h - l| <= 2^-22 |v| while no part is
// subnormal; the subtraction is exact in f32), and a product a b is the three partial products down to 2^-11 relative size
//
//     a_h b_l + a_l b_h + a_h b_h        (dropped: a_l b_l <= 2^-22 |a b|)
//
// on v_mfma_f32_16x16x32_f16 (f16 x f16 is exact in f32; f32 accumulation): HALF the matrix instructions, two thirds of the weight stream,
// LDS reads and conversions.  f16 has 5 exponent bits, so both operands are brought into its range by POWERS OF TWO (exact):
//   weights      layer l is stored as W_l 2^ew_l with max |W_l| 2^ew_l in [2^14, 2^15) (host: zuko_amd/fused.py, zk_gather_split_f16);
//   activations  every SAMPLE's input vector of a layer is scaled by 2^ea with max_k |a_k| 2^ea in [2^14, 2^15) before it is split (a lane
//                holds values of ONE sample; its four lanes agree on ea through two shuffles);
// and the accumulator returns through ONE fma:  out = fma(acc, 2^-(ew_l + ea), bias)  — products and sums before it carry no rounding but
// the f32 accumulation's.  Values more than 2^18 below their vector's maximum lose relative (not absolute) precision: an element's absolute
// error stays below 2^-40 of the vector's maximum.  Exponent bookkeeping: arh_scale.  Measured against float64 next to the reference's own f32 evaluation (random-init, x30
// "trained", 2^-120 / 2^100 scaled weights: scripts/split_scheme_emulation.py, tests/test_gpu_flows.py): the same error as the f32 path;
// weights whose magnitudes spread over more than the f16 range WITHIN a layer keep the three-part kernel (zuko_amd/fused.py: eligibility).
// A hidden value that overflows f32 becomes NaN for its sample, as in fused_ar_split_impl.h (inf - inf in the low part).
//
// Stream layout, raw reads and counted waits are those of fused_ar_split_impl.h with TWO 1 KiB images (h, l) per block; the frame around the
// matrix part (LDS carve-up, input stage, epilogue) is zk_ar_common.h's.  The ring is this header's: four slots with a chunk visible one chunk
// before it is read (ArhRing4) where they fit the LDS, else the three-slot ring of fused_ar_static_impl.h with a wait that knows the x loads (ArhRing).
#pragma once
#include "fused_ar_split_impl.h"

#ifndef ARH_LOOK
#define ARH_LOOK 1  // blocks of weight images requested ahead of the matrix instructions that consume them
#endif
#ifndef ARH_RELU_INT
#define ARH_RELU_INT 0  // probe builds: 1 = ReLU as an integer max (one instruction; a NaN with the sign bit set would become 0)
#endif
#ifndef ARH_EPI_PINNED
#define ARH_EPI_PINNED 1  // probe builds: 0 = the split and the ReLU as plain C++ (compare / select, convert back, subtract, convert)
#endif
#ifndef ARH_DESCALE_PK
#define ARH_DESCALE_PK 1  // probe builds: 0 = the hidden layers' descale as one v_fma_f32 per value (1: one v_pk_fma_f32 per pair)
#endif
#ifndef ARH_PREFETCH
#define ARH_PREFETCH 1  // probe builds: 0 = a tile's x rows and its log-derivative are requested where they are consumed
#endif
#ifndef ARH_BLOCK_ASM
#define ARH_BLOCK_ASM 1  // probe builds: 0 = a block's counted wait as an asm statement that defines the images, its matrix instructions the compiler's (arh_settle, arh_block: one s_nop between them)
#endif
#ifndef ARH_EPI_TILE
#define ARH_EPI_TILE 1  // probe builds: 0 = ReLU and the sample maximum of a hidden layer behind the whole layer (1: behind every out tile's descale, among the matrix instructions)
#endif

#ifndef ARH_SPLIT_GAPS
#define ARH_SPLIT_GAPS 1  // 0 = every in pair of a layer is split in front of the layer (1: pair p + 1 one instruction per gap among the matrix instructions of the blocks in front of its first reader: arh_gap_plan; profiles/half_gaps/README.md)
#endif

namespace zk {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct ArhB {  // B operand of one pair of activation tiles
  f16x8 h, l;
};

// power-of-two scale of a sample: s = 2^ea with amax * s in [2^14, 2^15) for amax in [2^-75, 2^105]; ea stays in [-90, 90] so that the accumulator's
// descale factor 2^-(ew + ea) (ew in [-25, 35]: zuko_amd/fused.py, half_scales) is a normal f32 number.  Beyond: a sample whose largest magnitude
// exceeds 2^105 (4e31) overflows f16 and becomes NaN — as a non-finite value does (inf - inf in the low part) —, smaller ones than 2^-75 lose
// relative precision (absolute error below 2^-100).  amax = 0: zeros stay zeros.
__device__ __forceinline__ void arh_scale(float& amax, float& s, float& inv_s) {  // (amax returns as the SAMPLE's maximum)
  amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
  amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
  int e = __builtin_amdgcn_frexp_expf(amax);  // amax = f 2^e, f in [0.5, 1); 0 for zero / inf / NaN
  int ea = 15 - e;
  ea = ea > 90 ? 90 : (ea < -90 ? -90 : ea);
  s = __builtin_amdgcn_ldexpf(1.0f, ea);
  inv_s = __builtin_amdgcn_ldexpf(1.0f, -ea);
}

// smallest sample maximum whose scaled value (ea = -90) rounds to an f16 infinity: from here on a sample is NaN (see above)
#define ARH_AMAX_OVERFLOW (65520.f * 0x1p90f)

typedef unsigned arh_u32x4 __attribute__((ext_vector_type(4)));
typedef float arh_f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void arh_split(const f32x4& lo, const f32x4& hi, float s, ArhB& b) {
  if (ARX_ABL == 6) {
    b.h = __builtin_bit_cast(f16x8, lo); b.l = __builtin_bit_cast(f16x8, hi);
    return;
  }
#if ARH_EPI_PINNED
  // TWO instructions per value, pinned (under -ffp-contract=off the compiler converts h back, subtracts and converts: four):
  //   h = f16(fma(v, s, -0))   v s is exact (s is a power of two) and -0 keeps the sign of a zero: the bits of (_Float16)(v * s)
  //   l = f16(fma(v, s, -h))   v s - h is exact in f32: the bits of (_Float16)(v * s - (float)h)
  // (v s below the f32 normal range: |v s| < 2^-126 gives h = 0 and l = 0 either way.)  mixlo / mixhi write one half of the destination.
  // ONE statement per call (sixteen single-instruction statements: the compiler pads a statement that reads what the one in front of it wrote).
  const float nz = -0.f;
  unsigned h0, h1, h2, h3, l0, l1, l2, l3;
#define ARH_SPLIT_H(OP, H, V) "v_fma_mix" OP "_f16 %[" H "], %[" V "], %[s], %[nz]\n\t"
#define ARH_SPLIT_L(OP, SEL, L, H, V) "v_fma_mix" OP "_f16 %[" L "], %[" V "], %[s], -%[" H "] op_sel:[0,0," SEL "] op_sel_hi:[0,0,1]\n\t"
  asm(ARH_SPLIT_H("lo", "h0", "v0") ARH_SPLIT_H("lo", "h1", "v2") ARH_SPLIT_H("lo", "h2", "v4") ARH_SPLIT_H("lo", "h3", "v6")
      ARH_SPLIT_H("hi", "h0", "v1") ARH_SPLIT_H("hi", "h1", "v3") ARH_SPLIT_H("hi", "h2", "v5") ARH_SPLIT_H("hi", "h3", "v7")
      ARH_SPLIT_L("lo", "0", "l0", "h0", "v0") ARH_SPLIT_L("lo", "0", "l1", "h1", "v2") ARH_SPLIT_L("lo", "0", "l2", "h2", "v4") ARH_SPLIT_L("lo", "0", "l3", "h3", "v6")
      ARH_SPLIT_L("hi", "1", "l0", "h0", "v1") ARH_SPLIT_L("hi", "1", "l1", "h1", "v3") ARH_SPLIT_L("hi", "1", "l2", "h2", "v5") ARH_SPLIT_L("hi", "1", "l3", "h3", "v7")
      : [h0] "=&v"(h0), [h1] "=&v"(h1), [h2] "=&v"(h2), [h3] "=&v"(h3), [l0] "=&v"(l0), [l1] "=&v"(l1), [l2] "=&v"(l2), [l3] "=&v"(l3)
      : [v0] "v"(lo[0]), [v1] "v"(lo[1]), [v2] "v"(lo[2]), [v3] "v"(lo[3]), [v4] "v"(hi[0]), [v5] "v"(hi[1]), [v6] "v"(hi[2]), [v7] "v"(hi[3]), [s] "v"(s), [nz] "s"(nz));
#undef ARH_SPLIT_H
#undef ARH_SPLIT_L
  b.h = __builtin_bit_cast(f16x8, arh_u32x4{h0, h1, h2, h3}); b.l = __builtin_bit_cast(f16x8, arh_u32x4{l0, l1, l2, l3});
  return;
#endif
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float v = (e < 4 ? lo[e] : hi[e - 4]) * s;
    const _Float16 h = (_Float16)v;
    const float r = v - (float)h;
    b.h[e] = h;
    b.l[e] = (_Float16)r;
  }
}

#define ARH_MFMA(A, B, C) C = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, A), B, C, 0, 0, 0)
// the three partial products of one block, smallest first (a[0] = h, a[1] = l image of the weights)
__device__ __forceinline__ void arh_block(const f32x4 (&a)[2], const ArhB& b, f32x4& c) {
  if (ARX_ABL == 2) {
    asm volatile("" ::"v"(a[0]), "v"(a[1]));
    return;
  }
  ARH_MFMA(a[1], b.h, c);
  ARH_MFMA(a[0], b.l, c);
  ARH_MFMA(a[0], b.h, c);
}

__device__ __forceinline__ void arh_touch(f32x4& v) { asm volatile("" : "+v"(v)); }  // a raw-read register becomes usable HERE (behind the counted wait that settled it)
template <int N> __device__ __forceinline__ void arh_settle(f32x4& a0, f32x4& a1) { asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a0), "+v"(a1) : "n"(N)); }
template <int N> __device__ __forceinline__ void arh_settle(f32x4& a0, f32x4& a1, f32x4& a2) { asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(a0), "+v"(a1), "+v"(a2) : "n"(N)); }

// A block without the compiler's pad: the counted wait that settles its weight images as the COMPILER's instruction (__builtin_amdgcn_s_waitcnt),
// the three partial products (arh_block's, in its order) as ONE statement behind it.  The compiler's hazard recogniser pads any asm statement, and
// any matrix instruction, that reads or writes a register an asm statement in front of it defined while nothing but asm statements stands between
// the two (they count as no wait state).  The raw weight reads are asm statements, so a wait written as an asm statement draws one s_nop per block,
// on whichever side of it the matrix instructions' statement begins; the builtin is an instruction of the compiler's own and is the one wait state
// the rule asks for.  Inside the string nothing is padded, so the wait states are written here:
//   FIRST  a tile's first block: the accumulator starts from the inline constant 0 (early-clobber: written before the last operand is read)
//   PAD    a layer's first block: its B operands may have been written by the vector instruction in front of the wait (arh_split), and a matrix
//          instruction reads a just-written operand two wait states later at the earliest: one more state in front of the wait
//   TILE   a hidden tile's last block: the bias tile `bs` counts as settled behind the wait (a raw read, as the images), and the twelve wait states
//          between the tile's last matrix instruction and the vector instruction that reads the accumulator (the descale) end the string
// (the last layer's groups place their twelve states themselves: arh_acc_ready).  The images are inputs: what orders the matrix instructions behind
// the wait is the statement order of a builtin with side effects and a volatile asm, and the scheduling fence between them.
constexpr bool ARH_BLK = ARH_BLOCK_ASM && ARX_ABL != 2;
// GAPS (ARH_SPLIT_GAPS): the block carries one form of an in pair's operand split, ONE v_fma_mix*_f16 behind each of its matrix instructions.  A
// v_mfma_f32_16x16x32_f16 holds the SIMD's vector issue for half of its time; with both wavefronts of a SIMD issuing matrix instructions one
// v_fma_mix*_f16 (or transcendental) or two v_fma_f32 / v_max_f32 / v_cndmask_b32 per gap cost 1.8 cycles per matrix instruction together, a
// second v_fma_mix*_f16 6.5 more, one packed f32 instruction 13.6 (scripts/probes/gap_fill_probe.hip, profiles/half_gaps/gap_fill_probe.txt).
// The sixteen instructions of arh_split, in its order, are the forms 1..6 (3, 3, 3, 3, 3, 1: the gap behind the last block of a split stays
// empty, so the pair's first reader never follows its last write directly); they work on the pair's eight registers as scalars (ArhHL).
constexpr bool ARH_GAPS = ARH_SPLIT_GAPS && ARH_BLK && ARH_EPI_PINNED && ARX_ABL != 6;
struct ArhHL {  // the registers of an ArhB while its split is under way
  unsigned h0, h1, h2, h3, l0, l1, l2, l3;
};
#define ARH_GH(OP, H, V) "\n\tv_fma_mix" OP "_f16 %[" H "], %[" V "], %[s], %[nz]"
#define ARH_GL(OP, SEL, L, H, V) "\n\tv_fma_mix" OP "_f16 %[" L "], %[" V "], %[s], -%[" H "] op_sel:[0,0," SEL "] op_sel_hi:[0,0,1]"
#define ARH_G0 ARH_GH("lo", "h0", "v0")
#define ARH_G1 ARH_GH("lo", "h1", "v2")
#define ARH_G2 ARH_GH("lo", "h2", "v4")
#define ARH_G3 ARH_GH("lo", "h3", "v6")
#define ARH_G4 ARH_GH("hi", "h0", "v1")
#define ARH_G5 ARH_GH("hi", "h1", "v3")
#define ARH_G6 ARH_GH("hi", "h2", "v5")
#define ARH_G7 ARH_GH("hi", "h3", "v7")
#define ARH_G8 ARH_GL("lo", "0", "l0", "h0", "v0")
#define ARH_G9 ARH_GL("lo", "0", "l1", "h1", "v2")
#define ARH_G10 ARH_GL("lo", "0", "l2", "h2", "v4")
#define ARH_G11 ARH_GL("lo", "0", "l3", "h3", "v6")
#define ARH_G12 ARH_GL("hi", "1", "l0", "h0", "v1")
#define ARH_G13 ARH_GL("hi", "1", "l1", "h1", "v3")
#define ARH_G14 ARH_GL("hi", "1", "l2", "h2", "v5")
#define ARH_G15 ARH_GL("hi", "1", "l3", "h3", "v7")
// operands per form: a register's first write is early-clobber (the statement reads other inputs behind it), the later ones update it
#define ARH_G_OUT0
#define ARH_G_IN0
#define ARH_G_SC [s] "v"(s), [nz] "s"(nz)
#define ARH_G_OUT1 , [h0] "=&v"(x.h0), [l0] "=&v"(x.l0)
#define ARH_G_IN1 , [v0] "v"(lo[0]), [v1] "v"(lo[1]), ARH_G_SC
#define ARH_G_OUT2 , [l0] "+v"(x.l0), [h1] "=&v"(x.h1)
#define ARH_G_IN2 , [v1] "v"(lo[1]), [h0] "v"(x.h0), [v2] "v"(lo[2]), [v3] "v"(lo[3]), ARH_G_SC
#define ARH_G_OUT3 , [l1] "=&v"(x.l1), [h2] "=&v"(x.h2)
#define ARH_G_IN3 , [v2] "v"(lo[2]), [v3] "v"(lo[3]), [h1] "v"(x.h1), [v4] "v"(hi[0]), ARH_G_SC
#define ARH_G_OUT4 , [h2] "+v"(x.h2), [l2] "=&v"(x.l2)
#define ARH_G_IN4 , [v5] "v"(hi[1]), [v4] "v"(hi[0]), ARH_G_SC
#define ARH_G_OUT5 , [h3] "=&v"(x.h3), [l3] "=&v"(x.l3)
#define ARH_G_IN5 , [v6] "v"(hi[2]), [v7] "v"(hi[3]), ARH_G_SC
#define ARH_G_OUT6 , [l3] "+v"(x.l3)
#define ARH_G_IN6 , [v7] "v"(hi[3]), [h3] "v"(x.h3), [s] "v"(s)
// the forms F..6 as one statement (F >= 2): what the forms in front of F have defined is updated or read, the rest is defined here — early-clobber
// as well: an update of a register nothing has defined yet may be given the register of an input the statement still reads
#define ARH_T_OUT2 [l0] "+v"(x.l0), [h1] "=&v"(x.h1), [l1] "=&v"(x.l1), [h2] "=&v"(x.h2), [l2] "=&v"(x.l2), [h3] "=&v"(x.h3), [l3] "=&v"(x.l3)
#define ARH_T_IN2 [v1] "v"(lo[1]), [v2] "v"(lo[2]), [v3] "v"(lo[3]), [v4] "v"(hi[0]), [v5] "v"(hi[1]), [v6] "v"(hi[2]), [v7] "v"(hi[3]), [h0] "v"(x.h0), ARH_G_SC
#define ARH_T_OUT3 [l1] "=&v"(x.l1), [h2] "=&v"(x.h2), [l2] "=&v"(x.l2), [h3] "=&v"(x.h3), [l3] "=&v"(x.l3)
#define ARH_T_IN3 [v2] "v"(lo[2]), [v3] "v"(lo[3]), [v4] "v"(hi[0]), [v5] "v"(hi[1]), [v6] "v"(hi[2]), [v7] "v"(hi[3]), [h1] "v"(x.h1), ARH_G_SC
#define ARH_T_OUT4 [h2] "+v"(x.h2), [l2] "=&v"(x.l2), [h3] "=&v"(x.h3), [l3] "=&v"(x.l3)
#define ARH_T_IN4 [v4] "v"(hi[0]), [v5] "v"(hi[1]), [v6] "v"(hi[2]), [v7] "v"(hi[3]), ARH_G_SC
#define ARH_T_OUT5 [h3] "=&v"(x.h3), [l3] "=&v"(x.l3)
#define ARH_T_IN5 [v6] "v"(hi[2]), [v7] "v"(hi[3]), ARH_G_SC
#define ARH_T_OUT6 [l3] "+v"(x.l3)
#define ARH_T_IN6 [v7] "v"(hi[3]), [h3] "v"(x.h3), [s] "v"(s)
#define ARH_BLK_ASM(C0, COUT, POST, BSOUT, G1, G2, G3, G)                                                   \
  asm volatile("v_mfma_f32_16x16x32_f16 %[c], %[al], %[bh], " C0 G1 "\n\t"                                  \
               "v_mfma_f32_16x16x32_f16 %[c], %[ah], %[bl], %[c]" G2 "\n\t"                                 \
               "v_mfma_f32_16x16x32_f16 %[c], %[ah], %[bh], %[c]" G3 POST                                   \
               : [c] COUT(c) ARH_BLK_BS##BSOUT ARH_G_OUT##G                                                 \
               : [ah] "v"(a[0]), [al] "v"(a[1]), [bh] "v"(b.h), [bl] "v"(b.l) ARH_G_IN##G)
#define ARH_BLK_BS0
#define ARH_BLK_BS1 , "+v"(bs)
#define ARH_BLK_FORM(G1, G2, G3, G)                                                               \
  if constexpr (FIRST && TILE) ARH_BLK_ASM("0", "=&v", "\n\ts_nop 11", 1, G1, G2, G3, G);          \
  else if constexpr (FIRST) ARH_BLK_ASM("0", "=&v", "", 0, G1, G2, G3, G);                         \
  else if constexpr (TILE) ARH_BLK_ASM("%[c]", "+v", "\n\ts_nop 11", 1, G1, G2, G3, G);            \
  else ARH_BLK_ASM("%[c]", "+v", "", 0, G1, G2, G3, G)
template <int N, bool FIRST, bool PAD, bool TILE> __device__ __forceinline__ void arh_wait_block(f32x4 (&a)[2], const ArhB& b, f32x4& c, f32x4& bs) {
  static_assert(N >= 0 && N < 16, "lgkmcnt is a four-bit field");
  if constexpr (PAD) asm volatile("s_nop 0");
  __builtin_amdgcn_s_waitcnt(0xC07F | (N << 8));  // lgkmcnt(N); vmcnt and expcnt at their maxima: not waited for
  if (ARX_FENCE) __builtin_amdgcn_sched_barrier(0);
  ARH_BLK_FORM("", "", "", 0);
  if (ARX_FENCE) __builtin_amdgcn_sched_barrier(0);
}
// the same block with form GF (1..6) of the split of (lo, hi) by the scale s in its gaps
template <int N, bool FIRST, bool PAD, bool TILE, int GF>
__device__ __forceinline__ void arh_wait_block(f32x4 (&a)[2], const ArhB& b, f32x4& c, f32x4& bs, ArhHL& x, const f32x4& lo, const f32x4& hi, float s) {
  static_assert(N >= 0 && N < 16 && GF >= 1 && GF <= 6, "lgkmcnt is a four-bit field; six forms");
  const float nz = -0.f;
  if constexpr (PAD) asm volatile("s_nop 0");
  __builtin_amdgcn_s_waitcnt(0xC07F | (N << 8));
  if (ARX_FENCE) __builtin_amdgcn_sched_barrier(0);
  if constexpr (GF == 1) { ARH_BLK_FORM(ARH_G0, ARH_G4, ARH_G8, 1); }
  else if constexpr (GF == 2) { ARH_BLK_FORM(ARH_G12, ARH_G1, ARH_G5, 2); }
  else if constexpr (GF == 3) { ARH_BLK_FORM(ARH_G9, ARH_G13, ARH_G2, 3); }
  else if constexpr (GF == 4) { ARH_BLK_FORM(ARH_G6, ARH_G10, ARH_G14, 4); }
  else if constexpr (GF == 5) { ARH_BLK_FORM(ARH_G3, ARH_G7, ARH_G11, 5); }
  else { ARH_BLK_FORM(ARH_G15, "", "", 6); }
  if (ARX_FENCE) __builtin_amdgcn_sched_barrier(0);
}
// the forms F..6 of a split as one statement: what found no block in front of the pair's first reader (all of it: arh_split)
template <int F> __device__ __forceinline__ void arh_split_tail(ArhHL& x, const f32x4& lo, const f32x4& hi, float s) {
  static_assert(F >= 2 && F <= 6, "six forms");
  const float nz = -0.f;
#define ARH_T6 ARH_G15
#define ARH_T5 ARH_G3 ARH_G7 ARH_G11 ARH_T6
#define ARH_T4 ARH_G6 ARH_G10 ARH_G14 ARH_T5
#define ARH_T3 ARH_G9 ARH_G13 ARH_G2 ARH_T4
#define ARH_T2 ARH_G12 ARH_G1 ARH_G5 ARH_T3
#define ARH_TAIL_ASM(T, F) asm("; the rest of a split" T : ARH_T_OUT##F : ARH_T_IN##F)
  if constexpr (F == 2) ARH_TAIL_ASM(ARH_T2, 2);
  else if constexpr (F == 3) ARH_TAIL_ASM(ARH_T3, 3);
  else if constexpr (F == 4) ARH_TAIL_ASM(ARH_T4, 4);
  else if constexpr (F == 5) ARH_TAIL_ASM(ARH_T5, 5);
  else ARH_TAIL_ASM(ARH_T6, 6);
#undef ARH_TAIL_ASM
#undef ARH_T2
#undef ARH_T3
#undef ARH_T4
#undef ARH_T5
#undef ARH_T6
}
// The eight registers become the pair's two operands HERE: where the compiler could not make them two register quads from the start it copies, and
// the copy has to stand in front of this statement — not in front of the block that reads the pair first, behind that block's wait, where the
// matrix instruction (inside a string, unseen by the hazard recogniser) would read the register in the copy's shadow.
__device__ __forceinline__ void arh_split_done(const ArhHL& x, ArhB& b) {
  b.h = __builtin_bit_cast(f16x8, arh_u32x4{x.h0, x.h1, x.h2, x.h3}); b.l = __builtin_bit_cast(f16x8, arh_u32x4{x.l0, x.l1, x.l2, x.l3});
  asm volatile("" : "+v"(b.h), "+v"(b.l));
}
#undef ARH_BLK_FORM
#undef ARH_BLK_ASM
#undef ARH_BLK_BS0
#undef ARH_BLK_BS1
#undef ARH_G_OUT0
#undef ARH_G_IN0
#undef ARH_G_OUT1
#undef ARH_G_IN1
#undef ARH_G_OUT2
#undef ARH_G_IN2
#undef ARH_G_OUT3
#undef ARH_G_IN3
#undef ARH_G_OUT4
#undef ARH_G_IN4
#undef ARH_G_OUT5
#undef ARH_G_IN5
#undef ARH_G_OUT6
#undef ARH_G_IN6
#undef ARH_G_SC
#undef ARH_T_OUT2
#undef ARH_T_IN2
#undef ARH_T_OUT3
#undef ARH_T_IN3
#undef ARH_T_OUT4
#undef ARH_T_IN4
#undef ARH_T_OUT5
#undef ARH_T_IN5
#undef ARH_T_OUT6
#undef ARH_T_IN6
#undef ARH_GH
#undef ARH_GL
#undef ARH_G0
#undef ARH_G1
#undef ARH_G2
#undef ARH_G3
#undef ARH_G4
#undef ARH_G5
#undef ARH_G6
#undef ARH_G7
#undef ARH_G8
#undef ARH_G9
#undef ARH_G10
#undef ARH_G11
#undef ARH_G12
#undef ARH_G13
#undef ARH_G14
#undef ARH_G15
// the accumulators of a last-layer group become readable: twelve wait states behind the group's last matrix instruction (the other tiles' last
// ones stand in front of it)
template <int NT> __device__ __forceinline__ void arh_acc_ready(f32x4 (&acc)[NT]) {
  asm volatile("s_nop 11" : "+v"(acc[NT - 1]));
#pragma unroll
  for (int t = 0; t + 1 < NT; ++t) arh_touch(acc[t]);
}

// ReLU of an out tile's four values and their entry into the sample maximum: ONE v_max_f32 per value, one v_max3_f32 per pair, a pair per statement.
// The maximum is kept as FOUR partial maxima (pm: non-negative, joined by arh_join_max) so that no v_max3_f32 waits for the one in front of it;
// max is exact, so the sample's maximum is the same bits in any order.  The max turns a NaN into 0, so no NaN may reach a hidden value: x, weights
// and biases are finite (poison; zuko_amd/fused.py: half_scales), products and sums of the f16 parts stay far inside f32, and the descale fma of
// finite operands gives a finite value or an infinity — which survives the max and is caught at the sample's maximum (arh_hidden_stack's poison:
// the next layer would compute inf - inf from it).
__device__ __forceinline__ void arh_relu_max(f32x4& o, float (&pm)[4], int t) {
#pragma unroll
  for (int r = 0; r < 4; r += 2)  // (pinned: behind a packed fma the compiler puts a canonicalising v_max in front of fmaxf)
    asm("v_max_f32 %0, 0, %0\n\tv_max_f32 %1, 0, %1\n\tv_max3_f32 %2, %2, %0, %1" : "+v"(o[r]), "+v"(o[r + 1]), "+v"(pm[(2 * t + r / 2) % 4]));
}
__device__ __forceinline__ float arh_join_max(const float (&pm)[4]) {
  float amax;
  asm("v_max_f32 %0, %1, %2\n\tv_max3_f32 %0, %0, %3, %4" : "=&v"(amax) : "v"(pm[0]), "v"(pm[1]), "v"(pm[2]), "v"(pm[3]));
  return amax;
}

// The ring of fused_ar_static_impl.h with a counted wait that knows about XV vector-memory loads YOUNGER than the chunk requested last (the
// next tile's x rows: arh_kernel).  Loads return in order: with the two youngest groups (XV loads, PER copies) still in flight, the chunk
// this advance hands to the readers has landed.  XV must be the number of load INSTRUCTIONS every wavefront has issued since the last
// advance, or fewer (a lower count only waits longer).
template <int WAVES, int CH, int NR> struct ArhRing : ArRingS<WAVES, CH, NR> {
  typedef ArRingS<WAVES, CH, NR> B;
  template <int XV> __device__ __forceinline__ void advance_x() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NR - 2) * B::PER + XV) : "memory");
    if (ARX_ABL != 4) __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    this->issue();
    this->slot = (this->slot + 1 == NR) ? 0 : this->slot + 1;
    this->cur_off = this->lds_off + (unsigned)(this->slot * CH * AR_TF * 4 + this->lane * 16);
  }
  template <int S, int XV = 0> __device__ __forceinline__ f32x4 read() {
    if constexpr (XV != 0 && S % CH == 0) {
      advance_x<XV>();
      f32x4 v;
      if (ARX_ABL == 5) {
        asm volatile("v_mov_b32 %0, %1" : "=v"(v[0]) : "v"(this->cur_off));
        v[1] = v[2] = v[3] = v[0];
        return v;
      }
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(this->cur_off), "n"((S % CH) * AR_TF * 4));
      return v;
    } else {
      return B::template read<S>();
    }
  }
};

// The FOUR-slot ring (Shape::NR == 4; zuko_amd/static_ar.py chooses it where four slots fit the LDS, and half_schedule there is this
// protocol as a list of events, checked by tests/test_half_ring_schedule.py).  Chunk g of the stream (counted on through the tiles) lives in
// slot g mod 4.  Its barrier B_g stands INSIDE the chunk, behind the request of the block at images BPOS, BPOS + 1:
//     wait, by vmcnt, for the wavefront's own pieces of chunk g + 2 (issued at B_(g-1): the only weight DMAs in flight)
//     barrier                                          -> chunk g + 2 is visible to every wavefront, a whole chunk before its first read
//     issue the pieces of chunk g + 3 into slot (g - 1) mod 4: every wavefront has SETTLED its last read of chunk g - 1 in front of B_g
//                                                         (BPOS >= 2 (ARH_LOOK + 1): the reads outstanding at B_g belong to chunk g)
// so no read waits at a barrier, a look-ahead request may cross the chunk boundary, and nothing drains the LDS queue.  Moving on to the next
// slot is one scalar add / compare / select and one vector add; the stream address is a scalar byte offset advanced by a constant and
// wrapped by one compare, the lane's 16-byte column a constant 32-bit vector offset.  Where the stream ends before image BPOS + 1 of its last
// chunk, B stands behind the chunk's last image and drains the LDS queue too (once per tile).  XV: as ArhRing's — vector-memory loads
// younger than the pieces waited for (the next tile's rows: arh_body's XPOS); every other B waits for vmcnt(0), a whole chunk after the
// request (the running log-derivative's load and a tile's stores, if still in flight, are sat out at the tile's first B).
template <int WAVES, int CH, int IMAGES, int BPOS, bool FLOW = false> struct ArhRing4 {
  static constexpr int NR = 4, PER = CH / WAVES, PIVOT = PER > 4 ? 4 : 0, CHB = CH * AR_TF * 4, NCH = (IMAGES + CH - 1) / CH;
  static_assert(PER * WAVES == CH && PER <= 6 && BPOS % 2 == 0 && BPOS >= 2 * (ARH_LOOK + 1) && BPOS + 1 < CH && CH % 2 == 0 && IMAGES % 2 == 0, "ring geometry");
  static constexpr int trigger(int c) {  // the image of chunk c behind whose request B stands (static_ar.half_trigger)
    const int last = (IMAGES < (c + 1) * CH ? IMAGES : (c + 1) * CH) - 1;
    return c * CH + BPOS + 1 < last ? c * CH + BPOS + 1 : last;
  }
  static constexpr int first_trigger_from(int pos) {  // the first B behind a load issued in front of the request of image pos
    for (int c = 0; c < NCH; ++c)
      if (trigger(c) >= pos) return trigger(c);
    return -1;
  }
  const char* gsrc;    // the stream + this wavefront's pieces of a chunk (scalar)
  char* ldst;          // the ring + the same
  unsigned goff, gend; // byte offset of the chunk requested next; bytes of the stream
  unsigned fill_off;   // byte offset of the slot it goes to
  unsigned read_off;   // byte offset of the slot being read
  unsigned lane_off;   // LDS byte address of the ring + lane * 16
  unsigned lane16;     // lane * 16
  unsigned cur_off;    // lane_off + read_off
  // FLOW (arhf_kernel: the passes of T transforms follow each other on one stream): whether the pass in progress requests the next tile's rows
  // (its XV boundary then leaves them in flight; in every other pass that boundary waits for vmcnt(0) like the rest), and the NEXT pass's bias
  // image — bias_n pieces of 1 KiB from bias_src to bias_dst (LDS), requested behind the barrier of the pass's last chunk but one, so that the
  // last chunk's barrier (which waits for everything but the rows) publishes it before the next pass reads its first bias tile
  bool rows_in_flight;
  const char* bias_src;
  char* bias_dst;
  int bias_n, wave_id;
  __device__ __forceinline__ void bias_request() {
    for (int p = wave_id; p < bias_n; p += WAVES)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bias_src + p * 1024 + (size_t)lane16), (__attribute__((address_space(3))) void*)(bias_dst + p * 1024), 16, 0, 0);
  }
  __device__ __forceinline__ void start(float* lds, const float* stream, int n_chunks, int wave, int lane) {
    const int b0 = wave * PER + PIVOT;
    gsrc = reinterpret_cast<const char*>(stream + b0 * AR_TF);
    ldst = reinterpret_cast<char*>(lds + b0 * AR_TF);
    goff = 0; gend = (unsigned)n_chunks * CHB; fill_off = 0;
    lane16 = (unsigned)lane * 16;
    lane_off = (unsigned)(size_t)((__attribute__((address_space(3))) float*)lds) + lane16;
    if constexpr (FLOW) { wave_id = wave; rows_in_flight = false; bias_n = 0; }
#pragma unroll
    for (int i = 0; i < NR - 1; ++i) issue();
    read_off = (NR - 1) * CHB;  // (the first read, position 0, moves on to slot 0)
    cur_off = lane_off;
  }
  template <int I> __device__ __forceinline__ void dma(const char* g, char* l) {
    if constexpr (I < PER) {
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, (I - PIVOT) * AR_TF * 4, 0);
      dma<I + 1>(g, l);
    }
  }
  __device__ __forceinline__ void issue() {
    asm volatile("" : "+v"(lane16));  // (kept apart from the scalar address: scalar base + 32-bit vector offset, no 64-bit vector add per chunk)
    if (ARX_ABL != 1) dma<0>(gsrc + goff + (size_t)lane16, ldst + fill_off);
    goff = (goff + CHB == gend) ? 0 : goff + CHB;
    fill_off = (fill_off + CHB == NR * CHB) ? 0 : fill_off + CHB;
  }
  template <int XV, bool DRAIN> __device__ __forceinline__ void wait() {
    if constexpr (DRAIN) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(XV) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(XV) : "memory");
  }
  template <int XV, bool DRAIN> __device__ __forceinline__ void boundary() {
    if constexpr (FLOW && XV != 0) {
      if (rows_in_flight) wait<XV, DRAIN>();
      else wait<0, DRAIN>();
    } else {
      wait<XV, DRAIN>();
    }
    if (ARX_ABL != 4) __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    issue();
    asm volatile("" ::: "memory");
  }
  template <int S, int XV = 0> __device__ __forceinline__ f32x4 read() {
    static_assert(S >= 0 && S < IMAGES, "stream position");
    if constexpr (S % CH == 0) {
      read_off = (read_off + CHB == NR * CHB) ? 0 : read_off + CHB;
      cur_off = lane_off + read_off;
    }
    f32x4 v;
    if (ARX_ABL == 5) {
      asm volatile("v_mov_b32 %0, %1" : "=v"(v[0]) : "v"(cur_off));
      v[1] = v[2] = v[3] = v[0];
    } else {
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(cur_off), "n"((S % CH) * AR_TF * 4));
    }
    if constexpr (S == trigger(S / CH)) boundary<XV, (S % CH != BPOS + 1)>();
    if constexpr (FLOW && NCH >= 2) {
      if constexpr (S == trigger(NCH - 2)) bias_request();
    }
    return v;
  }
};

// one hidden layer: out = fma(W' in', d, bias) over the blocks of the generated pattern (W', in': the scaled operands; d = 2^-(ew + ea))
template <class S, int L, bool ALT> constexpr int arh_ip(int s) {  // the in pair of block s of layer L
  if constexpr (ALT) return S::B_IP_ALT[s];
  else return ArxPat<S>::ip(L, s);
}
// (ALT, the flow kernel's first layer only: the blocks take the in pairs S::B_IP_ALT names — the pattern of the flow's OTHER feature order, which
//  differs from this one in nothing else)
// (EPI — the pinned ReLU path with ARH_EPI_TILE: an out tile's ReLU and its entry into the sample's partial maxima pm stand behind the tile's descale,
//  among the matrix instructions of the tiles that follow; nothing of them needs the whole layer)
template <class S> constexpr bool ARH_EPI = S::ACT == 1 && ARH_EPI_PINNED && ARH_EPI_TILE;

// Where the splits of a consuming layer's in pairs stand (ARH_SPLIT_GAPS).  L: a hidden layer 1..NH-1, or NH, the last layer (NT blocks per (group,
// in pair) step).  Its input is the layer before's output, still in `out`; the units are sorted by degree, so the layer's first blocks read the first
// in pairs only.  Pair 0 is split in front of the layer.  Pair p >= 1 takes the blocks from where pair p - 1 ended, one form per block, up to
// lim(p): the first block that reads the pair, or (hidden layers) the last block of the first out tile that overwrites out[2p] or out[2p + 1] —
// an out tile without blocks is written in front of the first block: lim 0.  The forms front(p)..6 found no block and stand in front of block lim(p).
template <int NBLK> struct ArhGapPlan {
  signed char pair[NBLK > 0 ? NBLK : 1], form[NBLK > 0 ? NBLK : 1];  // per block: the pair whose split it carries and the form (0: none)
  short lim[9];                                                      // per in pair
  signed char front[9];                                              // per in pair: 7 = nothing left over
};
template <class S, int L, int NT> constexpr int arh_gap_blocks() {
  if constexpr (L == S::NH) return S::GOFF[S::NG] * NT;
  else return S::NB[L];
}
template <class S, int L, int NT> constexpr int arh_gap_reader(int b) {  // the in pair block b reads
  if constexpr (L == S::NH) return S::G_IP[b / NT];
  else return ArxPat<S>::ip(L, b);
}
template <class S, int L> constexpr int arh_gap_last_block(int t) {  // the last block of out tile t of a hidden layer; -1: none, its bias is its value; NB: no such tile
  if (t >= S::HT[L]) return S::NB[L];
  int last = -1;
  for (int b = 0; b < S::NB[L]; ++b)
    if (ArxPat<S>::ot(L, b) == t) last = b;
  return last;
}
template <class S, int L, int NT> constexpr ArhGapPlan<arh_gap_blocks<S, L, NT>()> arh_gap_plan() {
  static_assert(L >= 1 && L <= S::NH && S::TMAX / 2 <= 8, "a consuming layer; eight in pairs at most");
  constexpr int NBLK = arh_gap_blocks<S, L, NT>(), NP = (S::HT[L - 1] + 1) / 2;
  ArhGapPlan<NBLK> g{};
  for (int p = 0; p < 9; ++p) { g.lim[p] = 0; g.front[p] = 7; }
  int cursor = 0;
  for (int p = 1; p < NP; ++p) {
    int lim = NBLK;
    for (int b = NBLK - 1; b >= 0; --b)
      if (arh_gap_reader<S, L, NT>(b) == p) lim = b;
    if constexpr (L != S::NH) {
      for (int t = 2 * p; t <= 2 * p + 1; ++t) {
        const int last = arh_gap_last_block<S, L>(t);
        lim = last < 0 ? 0 : (last < lim ? last : lim);
      }
    }
    int f = 1;
    for (; f <= 6 && cursor < lim; ++f, ++cursor) { g.pair[cursor] = (signed char)p; g.form[cursor] = (signed char)f; }
    g.lim[p] = (short)lim;
    g.front[p] = (signed char)f;
  }
  return g;
}
template <class S, int L, int NT, bool ON> struct ArhGapsOf {
  static constexpr int NP = 0, NBLK = 0;
  static constexpr int form(int) { return 0; }
  static constexpr int pair(int) { return 0; }
  static constexpr bool tail_at(int, int) { return false; }
  static constexpr bool any_tail_at(int) { return false; }
  static constexpr int front(int) { return 7; }
};
template <class S, int L, int NT> struct ArhGapsOf<S, L, NT, true> {
  static constexpr int NP = (S::HT[L - 1] + 1) / 2, NBLK = arh_gap_blocks<S, L, NT>();
  static constexpr ArhGapPlan<NBLK> plan = arh_gap_plan<S, L, NT>();
  static constexpr int form(int b) { return plan.form[b]; }
  static constexpr int pair(int b) { return plan.pair[b]; }
  static constexpr bool tail_at(int p, int b) { return p >= 1 && plan.front[p] <= 6 && plan.lim[p] == b; }  // pair p's leftover forms stand in front of block b (NBLK: behind the last block)
  static constexpr int front(int p) { return plan.front[p]; }
  static constexpr bool any_tail_at(int b) {
    for (int p = 1; p < NP; ++p)
      if (tail_at(p, b)) return true;
    return false;
  }
};
// the splits in front of the layer (pair 0, and every pair no block can carry), and those in front of block B (B >= 1; NBLK: behind the last block)
template <class GP, int HTI, int NPR> __device__ __forceinline__ void arh_gap_front(const f32x4 (&out)[2 * NPR], float s, ArhB (&in)[NPR]) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  arh_split(out[0], 1 < HTI ? out[1] : zero, s, in[0]);
  ars_for<GP::NP>([&](auto p_) ARS_ALWAYS_INLINE {
    constexpr int p = p_;
    if constexpr (GP::tail_at(p, 0)) arh_split(out[2 * p], 2 * p + 1 < HTI ? out[2 * p + 1] : zero, s, in[p]);
  });
}
template <class GP, int HTI, int B, int NPR> __device__ __forceinline__ void arh_gap_tails(ArhHL (&x)[NPR], const f32x4 (&out)[2 * NPR], float s, ArhB (&in)[NPR]) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  ars_for<GP::NP>([&](auto p_) ARS_ALWAYS_INLINE {
    constexpr int p = p_;
    if constexpr (B >= 1 && GP::tail_at(p, B)) {
      if constexpr (GP::front(p) == 1) {
        arh_split(out[2 * p], 2 * p + 1 < HTI ? out[2 * p + 1] : zero, s, in[p]);
      } else {
        arh_split_tail<GP::front(p)>(x[p], out[2 * p], 2 * p + 1 < HTI ? out[2 * p + 1] : zero, s);
        arh_split_done(x[p], in[p]);
      }
    }
  });
}

// GAPS (hidden layers 1..NH-1 with ARH_SPLIT_GAPS): `out` holds the layer's INPUT, to be split by the scale s_in into `in` as the blocks go
// (arh_gap_plan), and receives the layer's output tile by tile
template <class S, int L, class Ring, bool ALT = false, bool GAPS = false>
__device__ __forceinline__ void arh_hidden(Ring& ring, const float* bias_q, ArhB (&in)[S::TMAX / 2], f32x4 (&out)[S::TMAX], float d, float (&pm)[4], float s_in = 0.f) {
  typedef ArxPat<S> P;
  typedef ArhGapsOf<S, L, 0, GAPS> GP;
  constexpr int NB = S::NB[L], BASE = S::BASE[L], HTL = S::HT[L], HTI = S::HT[L > 0 ? L - 1 : 0];
  ArhHL x[S::TMAX / 2];
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if constexpr (GAPS) arh_gap_front<GP, HTI>(out, s_in, in);
  ars_for<HTL>([&](auto t_) ARS_ALWAYS_INLINE {
    constexpr int t = t_;
    if constexpr (!P::tile_has_blocks(L, t)) {
      out[t] = *reinterpret_cast<const f32x4*>(bias_q + t * 16);  // units that depend on nothing: bias only
      if constexpr (ARH_EPI<S>) arh_relu_max(out[t], pm, t);
    }
  });
  if constexpr (NB > 0) {
    constexpr int LOOK = ARH_LOOK < NB ? ARH_LOOK : NB;
    f32x4 a[LOOK + 1][2];
    f32x4 bs;  // the out tile's bias: a raw read in front of the look-ahead request of the tile's LAST block, whose counted wait settles it
    f32x4 acc;
    const unsigned bias_addr = arx_lds_addr(bias_q);
    ars_for<LOOK>([&](auto b_) ARS_ALWAYS_INLINE {
      constexpr int b = b_;
      ars_for<2>([&](auto p) ARS_ALWAYS_INLINE { a[b][p] = ring.template read<BASE + 2 * b + decltype(p)::value>(); });
    });
    ars_for<NB>([&](auto s_) ARS_ALWAYS_INLINE {
      constexpr int s = s_, ot = P::ot(L, s), cur = s % (LOOK + 1);
      constexpr int ip = arh_ip<S, L, ALT>(s);
      constexpr bool first_of_tile = (s == 0 || P::ot(L, s - 1) != ot), last_of_tile = (s + 1 == NB || P::ot(L, s + 1) != ot);
      if constexpr (first_of_tile && !ARH_BLK) acc = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (last_of_tile) bs = arx_lds_raw<ot * 64>(bias_addr);
      if constexpr (s + LOOK < NB) {
        constexpr int nx = (s + LOOK) % (LOOK + 1);
        ars_for<2>([&](auto p) ARS_ALWAYS_INLINE { a[nx][p] = ring.template read<BASE + 2 * (s + LOOK) + decltype(p)::value>(); });
      }
      constexpr int ahead = (s + LOOK < NB ? LOOK : NB - 1 - s);  // blocks behind this one whose images may still be outstanding
      // (a tile's last block: only THIS step's request is younger than the bias read — the wait that settles it also settles the blocks in between)
      if constexpr (GAPS) arh_gap_tails<GP, HTI, s>(x, out, s_in, in);  // (what found no block in front of this one, its first reader or the last of an out tile that overwrites the pair)
      constexpr int WAIT = last_of_tile ? (s + LOOK < NB ? 2 : 0) : 2 * ahead;
      constexpr bool pad = s == 0 || (GAPS && s >= 1 && GP::any_tail_at(s));
      if constexpr (GP::form(s) != 0) {
        constexpr int gp = GP::pair(s);
        arh_wait_block<WAIT, first_of_tile, pad, last_of_tile, GP::form(s)>(a[cur], in[ip], acc, bs, x[gp], out[2 * gp], 2 * gp + 1 < HTI ? out[2 * gp + 1] : zero, s_in);
        if constexpr (GP::form(s) == 6) arh_split_done(x[gp], in[gp]);
      } else if constexpr (ARH_BLK) {
        arh_wait_block<WAIT, first_of_tile, pad, last_of_tile>(a[cur], in[ip], acc, bs);
      } else {
        if constexpr (last_of_tile) arh_settle<(s + LOOK < NB ? 2 : 0)>(a[cur][0], a[cur][1], bs);
        else arh_settle<2 * ahead>(a[cur][0], a[cur][1]);
        if (ARX_FENCE) __builtin_amdgcn_sched_barrier(0);
        arh_block(a[cur], in[ip], acc);
        if (ARX_FENCE) __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (last_of_tile) {
        if (ARH_DESCALE_PK) {
#pragma unroll
          for (int r = 0; r < 4; r += 2) {
            const arh_f32x2 o = __builtin_elementwise_fma(arh_f32x2{acc[r], acc[r + 1]}, arh_f32x2{d, d}, arh_f32x2{bs[r], bs[r + 1]});
            out[ot][r] = o[0]; out[ot][r + 1] = o[1];
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) out[ot][r] = __builtin_fmaf(acc[r], d, bs[r]);
        }
        if constexpr (ARH_EPI<S>) arh_relu_max(out[ot], pm, ot);
      }
    });
    if constexpr (GAPS) arh_gap_tails<GP, HTI, NB>(x, out, s_in, in);
  }
}

// (wd: the per-layer descale factors 2^-ew_l of the stream being read — ArArgs::wdescale, or the transform's row of the flow kernel's table)
// HAS_ALT / alt (flow kernel): this pass's first layer follows S::B_IP_ALT
// s (ARH_SPLIT_GAPS): the scale by which the CONSUMER of a layer's output splits it — the next hidden layer (arh_hidden's GAPS) or, behind the last
// hidden layer, arh_pass; without the switch every layer's output is split here, behind the layer
template <class S, int L, class Ring, bool HAS_ALT = false> __device__ __forceinline__ void arh_hidden_stack(Ring& ring, const float* bias_lds, int q, ArhB (&in)[S::TMAX / 2], f32x4 (&out)[S::TMAX], const float* wd,
                                                                                                         float& inv_s, float& poison, float& s, bool alt = false) {
  if constexpr (L < S::NH) {
    float pm[4] = {0.f, 0.f, 0.f, 0.f};  // partial maxima of the layer's ReLU outputs (the pinned ReLU path: arh_relu_max)
    if constexpr (HAS_ALT && L == 0) {
      static_assert(S::BASE[0] == 0, "B_IP_ALT lists the first layer's blocks");
      if (alt) arh_hidden<S, L, Ring, true>(ring, bias_lds + L * S::BIAS_STRIDE + 4 * q, in, out, wd[L] * inv_s, pm);
      else arh_hidden<S, L, Ring>(ring, bias_lds + L * S::BIAS_STRIDE + 4 * q, in, out, wd[L] * inv_s, pm);
    } else {
      arh_hidden<S, L, Ring, false, ARH_GAPS && L >= 1>(ring, bias_lds + L * S::BIAS_STRIDE + 4 * q, in, out, wd[L] * inv_s, pm, s);
    }
    constexpr int HTL = S::HT[L];
    float amax = 0.f;
    if constexpr (S::ACT == 1 && ARH_EPI_PINNED) {
      // (arh_relu_max: with ARH_EPI_TILE every tile has been through it inside arh_hidden)
      if constexpr (!ARH_EPI_TILE) {
#pragma unroll
        for (int t = 0; t < HTL; ++t) arh_relu_max(out[t], pm, t);
      }
      amax = arh_join_max(pm);
    } else if constexpr (S::ACT == 1) {
#pragma unroll
      for (int t = 0; t < HTL; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (ARH_RELU_INT) out[t][r] = __builtin_bit_cast(float, max(__builtin_bit_cast(int, out[t][r]), 0));
          else out[t][r] = out[t][r] < 0.f ? 0.f : out[t][r];  // NaN stays NaN, as torch.relu
          amax = fmaxf(amax, out[t][r]);                  // (non-negative after the ReLU; a NaN is skipped here and poisons through the split)
        }
    } else {
      ar_activate<S::ACT, HTL>(out, out);
#pragma unroll
      for (int t = 0; t < HTL; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) amax = fmaxf(amax, fabsf(out[t][r]));
    }
    arh_scale(amax, s, inv_s);
    if constexpr (S::ACT == 1 && ARH_EPI_PINNED) {
      if (!(amax < ARH_AMAX_OVERFLOW)) poison = __builtin_nanf("");  // a hidden value overflowed f32 (or f16 after the scaling): NaN for its sample
    }
    if constexpr (!ARH_GAPS) {
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int p = 0; p < (HTL + 1) / 2; ++p) arh_split(out[2 * p], 2 * p + 1 < HTL ? out[2 * p + 1] : zero, s, in[p]);
    }
    arh_hidden_stack<S, L + 1, Ring, HAS_ALT>(ring, bias_lds, q, in, out, wd, inv_s, poison, s, alt);
  }
}

// One PASS of a row tile through the conditioner and the univariate map: the body of arh_body's tile loop, and of the flow kernel's loop over the
// transforms of a tile (FLOW; arhf_body).  wd: the stream's per-layer descale factors.  FLOW differs at the edges only: the rows come from the LDS row
// tile (the tile's x in the first pass, the y of the pass before in the others) and y goes back to it; the next tile's rows are requested in the tile's
// last pass; the log-derivative is added to `total` (a register) and stored, with the rows, behind the last pass — or, term, the last pass ends in
// the base's log-density and no rows are written.  The matrix part and the arithmetic of the epilogue are the same lines for both.
template <typename Uni> __device__ __forceinline__ void arh_flow_epilogue(float (&p)[4 * Uni::NT], const ArArgs& a, const int (&fid)[Uni::FPL], const float (&xin)[Uni::FPL], float poison, float* xr,
                                                                          const float* base, int D, bool term, float& lacc) {
  constexpr int FPL = Uni::FPL, TOTAL = Uni::TOTAL;
#pragma unroll
  for (int fi = 0; fi < FPL; ++fi) Uni::template poison<false>(p, fi * TOTAL, poison);
  auto ld = [&](int i) { return p[i]; };
#pragma unroll
  for (int fi = 0; fi < FPL; ++fi) {
    const int f = fid[fi];
    if (f >= 0) {
      float yv, lj;
      Uni::fwd(ld, fi * TOTAL, a, xin[fi], yv, lj);
      lacc += lj;
      if (term) {  // (ar_uni_epilogue's TERM branch with the base's table entries read here: ArLds::stage_base)
        const float df = yv - base[f];
        lacc += __builtin_fmaf(-(df * df), base[D + f], base[2 * D + f]);
      } else {
        xr[f] = yv;
      }
    }
  }
}

template <class S, typename Uni, bool DIAG, bool TERM, bool FLOW, class Ring, class XReq, class Fids>
__device__ __forceinline__ void arh_pass(const ArArgs& a, Ring& ring, XReq& x_request, f32x4 (&xnext)[S::NIT], float* bias_lds, const Fids& fids, float* xr, const float* base, const ArLane& ln,
                                         int64_t tile, const float* wd, bool first, bool last, bool term, float& total, bool alt = false) {
  constexpr bool RING4 = S::NR == 4;
  static_assert(!FLOW || (RING4 && S::XLDS && S::DIN == S::D && !DIAG && !TERM), "flow pass: four-slot ring, rows in LDS, no context columns");
  constexpr int NT = Uni::NT, FPL = Uni::FPL, WAVES = S::WAVES;
  constexpr int NG = S::NG;
  constexpr int NSTEP = S::GOFF[NG];  // (group, in pair) steps of the last layer, NT blocks each
  constexpr bool XLDS = S::XLDS;
  const int wave = ln.wave, j = ln.j, q = ln.q;
  const float* bias_last = bias_lds + S::NH * S::BIAS_STRIDE;
  const unsigned bias_last_addr = arx_lds_addr(bias_last + 4 * q);
  if constexpr (FLOW) {  // (the row tile was written by this wavefront's other lanes: ar_rows_in, or the pass before)
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  }
  const int64_t n = tile * (16 * WAVES) + wave * 16 + j;
  const bool live = n < a.N;
  const int64_t nc = live ? n : a.N - 1;
  const float* xrow = a.x + nc * a.ldx;

  ArhB in[S::TMAX / 2];
  f32x4 out[S::TMAX];
  float poison;
  float inv_s;  // 2^-ea of the operands `in` currently holds
  {
    f32x4 xin[S::NIT + 1];
#pragma unroll
    for (int it = 0; it < S::NIT; ++it) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if constexpr (FLOW) {  // (the row tile holds them: the tile's rows, or the y of the transform before this one)
        if ((it + 1) * 16 <= S::DIN || it * 16 + 4 * q < S::DIN) v = *reinterpret_cast<const f32x4*>(xr + it * 16 + 4 * q);
      } else if (ARH_PREFETCH) {
        if ((it + 1) * 16 <= S::DIN || it * 16 + 4 * q < S::DIN) v = xnext[it];
      } else {
        if ((it + 1) * 16 <= S::DIN || it * 16 + 4 * q < S::DIN) v = *reinterpret_cast<const f32x4*>(xrow + it * 16 + 4 * q);
      }
      xin[it] = v;
    }
    xin[S::NIT] = f32x4{0.f, 0.f, 0.f, 0.f};
    poison = ar_poison_of<S::NIT>(xin);
    float amax = 0.f;
#pragma unroll
    for (int it = 0; it < S::NIT; ++it)
#pragma unroll
      for (int r = 0; r < 4; ++r) amax = fmaxf(amax, fabsf(xin[it][r]));
    if constexpr (XLDS && !FLOW) ar_rows_in<S::D>(xr, q, xin);
    float s;
    arh_scale(amax, s, inv_s);
    if constexpr (S::ACT == 1 && ARH_EPI_PINNED) {
      if (!(amax < ARH_AMAX_OVERFLOW)) poison = __builtin_nanf("");  // (finite, but its f16 parts are not: the one-instruction ReLU would flatten the NaN they make)
    }
#pragma unroll
    for (int p = 0; p < (S::NIT + 1) / 2; ++p) arh_split(xin[2 * p], xin[2 * p + 1], s, in[p]);
  }

  float ladj_in = 0.f;  // the running log-derivative this launch adds to: requested HERE, a whole tile ahead of the add
  if constexpr (!FLOW) {
    if (ARH_PREFETCH && a.ladj && a.accumulate && live && q == 0) ladj_in = a.ladj[n];
  }

  // ---- hidden layers ---------------------------------------------------------------------------------------------
  float s_last = 0.f;  // (ARH_SPLIT_GAPS: the scale of the last hidden layer's output, split under the last layer's blocks)
  if constexpr (FLOW) arh_hidden_stack<S, 0, Ring, S::FLOW_ALT>(ring, bias_lds, q, in, out, wd, inv_s, poison, s_last, alt);
  else arh_hidden_stack<S, 0, Ring>(ring, bias_lds, q, in, out, wd, inv_s, poison, s_last);
  typedef ArhGapsOf<S, S::NH, Uni::NT, (ARH_GAPS && S::NH >= 1)> GP;
  constexpr int HTI = S::HT[S::NH >= 1 ? S::NH - 1 : 0];
  ArhHL hl[S::TMAX / 2];
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if constexpr (ARH_GAPS && S::NH >= 1) arh_gap_front<GP, HTI>(out, s_last, in);

  // ---- last layer + univariate transform, one group of 4 * FPL features at a time --------------------------------
  const float dl = wd[S::NH] * inv_s;
  float lacc = 0.f;
  constexpr int NBL = NSTEP * NT;                          // blocks of the last layer
  constexpr int LOOKL = ARH_LOOK < NBL ? ARH_LOOK : NBL;
  f32x4 w[LOOKL + 1][2];
  // the next tile of this workgroup: its rows travel during the last layer.  The LAST tile requests its own rows again, so that the
  // count of loads in flight does not depend on the tile; XPOS is the one advance of the ring that finds them younger than its chunk
  // (four-slot ring: the first barrier behind the last layer's first request)
  constexpr int XPOS = []() constexpr {
    if constexpr (!ARH_PREFETCH) return -1;
    else if constexpr (RING4) return Ring::first_trigger_from(S::LAST_BASE);
    else return (S::LAST_BASE + S::CH - 1) / S::CH * S::CH;
  }();
  if constexpr (FLOW) {
    // the rows travel during the tile's LAST pass only; every other pass gives xnext a fresh (undefined) value instead, so that the registers
    // are free from the tile's start to here
    asm volatile("" ::: "memory");
    if (last) {
      x_request(tile + gridDim.x < a.n_tiles ? tile + gridDim.x : tile, xnext);
    } else {
#pragma unroll
      for (int it = 0; it < S::NIT; ++it) asm("" : "=v"(xnext[it]));
    }
    ring.rows_in_flight = last;
    asm volatile("" ::: "memory");
  } else if (ARH_PREFETCH) {
    asm volatile("" ::: "memory");
    x_request(tile + gridDim.x < a.n_tiles ? tile + gridDim.x : tile, xnext);
    asm volatile("" ::: "memory");
  }
#define ARH_READ_LAST(POS) ring.template read<(POS), ((POS) == XPOS ? S::NIT : 0)>()
  ars_for<LOOKL>([&](auto b_) ARS_ALWAYS_INLINE {
    constexpr int b = b_;
    ars_for<2>([&](auto p) ARS_ALWAYS_INLINE { w[b][p] = ARH_READ_LAST(S::LAST_BASE + 2 * b + decltype(p)::value); });
  });
  ars_for<NG>([&](auto g_) ARS_ALWAYS_INLINE {
    constexpr int g = g_, ST0 = S::GOFF[g], GN = S::GOFF[g + 1] - S::GOFF[g];
    int fid[FPL];
    float xin[FPL];
    fids.template fetch<XLDS>(g, xr, xrow, fid, xin);
    float bv[3 * FPL];
    if constexpr (TERM && !FLOW) fids.fetch_base(fid, base, S::D, bv);
    f32x4 acc[NT], bs[NT];  // the group's bias tiles: raw reads in front of the look-ahead request of the group's LAST block, whose counted wait settles them
    if constexpr (GN == 0) {
      const float* bg = bias_last + (g * NT) * 16 + 4 * q;
      ars_for<NT>([&](auto t) ARS_ALWAYS_INLINE { bs[t] = *reinterpret_cast<const f32x4*>(bg + t * 16); });
    }
    if constexpr (GN == 0 || !ARH_BLK) ars_for<NT>([&](auto t) ARS_ALWAYS_INLINE { acc[t] = f32x4{0.f, 0.f, 0.f, 0.f}; });
    ars_for<GN>([&](auto i_) ARS_ALWAYS_INLINE {
      constexpr int st = ST0 + decltype(i_)::value, ip = S::G_IP[st];
      ars_for<NT>([&](auto t_) ARS_ALWAYS_INLINE {
        constexpr int t = t_, blk = st * NT + t, cur = blk % (LOOKL + 1);
        constexpr bool last_of_group = (decltype(i_)::value == GN - 1 && t == NT - 1);
        if constexpr (last_of_group) {
          ars_for<NT>([&](auto u) ARS_ALWAYS_INLINE { bs[u] = arx_lds_raw<(g * NT + decltype(u)::value) * 64>(bias_last_addr); });
        }
        if constexpr (blk + LOOKL < NBL) {
          constexpr int nx = (blk + LOOKL) % (LOOKL + 1);
          ars_for<2>([&](auto p) ARS_ALWAYS_INLINE { w[nx][p] = ARH_READ_LAST(S::LAST_BASE + 2 * (blk + LOOKL) + decltype(p)::value); });
        }
        constexpr int ahead = (blk + LOOKL < NBL ? LOOKL : NBL - 1 - blk);
        if constexpr (ARH_GAPS && S::NH >= 1) arh_gap_tails<GP, HTI, blk>(hl, out, s_last, in);  // (what found no block in front of this one, the pair's first reader)
        constexpr int WAIT = last_of_group ? (blk + LOOKL < NBL ? 2 : 0) : 2 * ahead;
        constexpr bool pad = blk == 0 || (ARH_GAPS && S::NH >= 1 && blk >= 1 && GP::any_tail_at(blk));
        if constexpr (ARH_BLK) {
          if constexpr (GP::form(blk) != 0) {
            constexpr int gp = GP::pair(blk);
            arh_wait_block<WAIT, decltype(i_)::value == 0, pad, false, GP::form(blk)>(w[cur], in[ip], acc[t], bs[0], hl[gp], out[2 * gp], 2 * gp + 1 < HTI ? out[2 * gp + 1] : zero, s_last);
            if constexpr (GP::form(blk) == 6) arh_split_done(hl[gp], in[gp]);
          } else {
            arh_wait_block<WAIT, decltype(i_)::value == 0, pad, false>(w[cur], in[ip], acc[t], bs[0]);
          }
          if constexpr (last_of_group) {  // (the bias tiles are older than this step's request: the block's wait has settled them)
#pragma unroll
            for (int u = 0; u < NT; ++u) arh_touch(bs[u]);
            arh_acc_ready<NT>(acc);
          }
        } else {
          if constexpr (last_of_group) arh_settle<(blk + LOOKL < NBL ? 2 : 0)>(w[cur][0], w[cur][1]);
          else arh_settle<2 * ahead>(w[cur][0], w[cur][1]);
          if constexpr (last_of_group) {  // (the bias tiles are older than this step's request: the same wait has settled them)
#pragma unroll
            for (int u = 0; u < NT; ++u) arh_touch(bs[u]);
          }
          if (ARX_FENCE) __builtin_amdgcn_sched_barrier(0);
          arh_block(w[cur], in[ip], acc[t]);
          if (ARX_FENCE) __builtin_amdgcn_sched_barrier(0);
        }
      });
    });
    float p[4 * NT];
    ars_for<NT>([&](auto t) ARS_ALWAYS_INLINE {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[4 * t + r] = __builtin_fmaf(acc[t][r], dl, bs[t][r]);
        // one fma per parameter, written where the spline wants it: left alone, the vectoriser pairs parameter j with parameter K + j (the
        // spline's two axes) in FRONT of the fma and gathers accumulator and bias elements into register pairs for it (3 v_mov per pair)
        if (ARH_POISON_ONE) asm("" : "+v"(p[4 * t + r]));
      }
    });
    if constexpr (FLOW) arh_flow_epilogue<Uni>(p, a, fid, xin, poison, xr, base, S::D, last && term, lacc);
    else ar_uni_epilogue<Uni, DIAG, XLDS, true, TERM>(p, a, fid, xin, poison, xr, n, live, S::D, lacc, bv);
  });
#undef ARH_READ_LAST
  if constexpr (ARH_GAPS && S::NH >= 1) arh_gap_tails<GP, HTI, NBL>(hl, out, s_last, in);  // (pairs no block reads)
  if constexpr (FLOW) {
    // the transform's log-derivative joins the running sum as a launch of its own would add it to the buffer: summed over the sample's four lanes first
    lacc += __shfl_xor(lacc, 16, 64);
    lacc += __shfl_xor(lacc, 32, 64);
    total = first ? lacc : total + lacc;
    if (last) {
      if (live && q == 0) a.ladj[n] = total;
      if (!term) ar_rows_out<S::D>(xr, q, a.y + n * a.ldy, live);
    }
    return;
  }
  if (ARH_PREFETCH) ar_ladj_store<true>(a, lacc, n, live, q, ladj_in);  // in FRONT of the y rows: the wait for ladj_in (requested a tile ago) must not find stores it would have to sit out
  if constexpr (XLDS && !TERM) ar_rows_out<S::D>(xr, q, a.y + n * a.ldy, live);
  if (!ARH_PREFETCH) ar_ladj_store(a, lacc, n, live, q);
}

// The kernel's body.  DIAG: the diagnostic twin of the product launch (also writes the bin index the spline USED and the knots it searched), as
// arx_kernel's.  TERM: the terminal launch of a log_prob (arht_kernel): the base's tables staged behind the feature map, no y rows written, the
// log-density in the ladj buffer (zk_ar_common.h: ArArgs::base_loc).
template <class S, typename Uni, bool DIAG, bool TERM> __device__ __forceinline__ void arh_body(const ArArgs& a) {
  constexpr bool RING4 = S::NR == 4;
  typedef std::conditional_t<RING4, ArhRing4<S::WAVES, S::CH, S::IMAGES, S::BPOS>, ArhRing<S::WAVES, S::CH, S::NR>> Ring;
  static_assert(S::WAVES == 8 && (S::NR == 3 || S::NR == 4) && S::TMAX <= 16 && S::TMAX % 2 == 0 && S::OCC == 2, "two-part split kernels: widths <= 256, two wavefronts per SIMD");
  constexpr int NT = Uni::NT, FPL = Uni::FPL, WAVES = S::WAVES;
  constexpr int NG = S::NG;
  constexpr int NSTEP = S::GOFF[NG];  // (group, in pair) steps of the last layer, NT blocks each
  static_assert(S::IMAGES == S::LAST_BASE + 2 * NSTEP * NT && (S::IMAGES + S::CH - 1) / S::CH == S::NCHUNK, "stream length");
  const ArLane ln;
  const int tid = ln.tid, lane = ln.lane, wave = ln.wave, j = ln.j, q = ln.q;

  Ring ring;
  if constexpr (RING4) {
    ring.start(ars_lds, a.stream, a.n_chunks, wave, lane);
  } else {
    // (ArRingS::start written out: called as the member, this kernel's first two requests come out with scalar base addresses and the loop's vector
    //  base is built a second time — one vector instruction more, profiles/ar_frame/census.md)
    ring.lds = ars_lds; ring.stream = a.stream; ring.n_chunks = a.n_chunks; ring.wave = wave; ring.lane = lane;
    ring.load_chunk = 0; ring.load_slot = 0;
#pragma unroll
    for (int i = 0; i < S::NR - 1; ++i) ring.issue();
    ring.slot = S::NR - 1;
    ring.lds_off = (unsigned)(size_t)((__attribute__((address_space(3))) float*)ars_lds);
    ring.cur_off = ring.lds_off;
  }

  // x rows of a tile, 4 values of S::NIT 16-column groups per lane.  Every lane loads (a column group that ends beyond DIN is read at the
  // row's last four columns and zeroed afterwards): the number of load instructions in flight is the same for every wavefront (ArhRing)
  auto x_request = [&](int64_t tile, f32x4 (&xv)[S::NIT]) ARS_ALWAYS_INLINE {
    const int64_t n = tile * (16 * WAVES) + wave * 16 + j;
    const float* row = a.x + (n < a.N ? n : a.N - 1) * a.ldx;
#pragma unroll
    for (int it = 0; it < S::NIT; ++it) {
      const int col = it * 16 + 4 * q;
      xv[it] = *reinterpret_cast<const f32x4*>(row + ((it + 1) * 16 <= S::DIN || col < S::DIN ? col : S::DIN - 4));
    }
  };
  f32x4 xnext[S::NIT];  // the NEXT tile's rows: requested a last layer ahead of the tile that consumes them
  if (ARH_PREFETCH) x_request(blockIdx.x, xnext);  // (the first tile's: landed behind the barrier below)

  float* const bias_lds = ars_lds + S::NR * S::CH * AR_TF;
  int* const fmap_lds = ArLds::fmap(bias_lds, a.bias_floats);
  float* const xr = ArLds::row(fmap_lds, wave, j, a.xs);
  float* const base = ArLds::base(fmap_lds, NG * 4 * FPL);
  if constexpr (TERM) ArLds::stage_base<64 * WAVES>(a, tid, base, S::D);
  ArLds::stage<64 * WAVES>(a, tid, bias_lds, fmap_lds, NG * 4 * FPL);
  const ArFids<NG, FPL, (NG * FPL <= 32)> fids(fmap_lds, q);

  float unused = 0.f;
  for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x)
    arh_pass<S, Uni, DIAG, TERM, false>(a, ring, x_request, xnext, bias_lds, fids, xr, base, ln, tile, a.wdescale, true, true, TERM, unused);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // look-ahead DMAs must land before the LDS is released
}

template <class S, typename Uni, bool DIAG = false> __global__ __launch_bounds__(64 * S::WAVES, S::OCC) void arh_kernel(ArArgs a) { arh_body<S, Uni, DIAG, false>(a); }
// (a name of its own: tests/test_codegen_half.py counts and bounds the arh_kernel instantiations of a generated unit)
template <class S, typename Uni> __global__ __launch_bounds__(64 * S::WAVES, S::OCC) void arht_kernel(ArArgs a) { arh_body<S, Uni, false, true>(a); }

template <class S, typename Uni> static int arh_launch(const ArArgs* in, int abi, int args_bytes, int train, void* stream) {
  if (abi != ARS_ABI || args_bytes != (int)sizeof(ArArgs)) return ZK_EINVAL;  // kernel built against another version of the library
  ArArgs a = *in;
  if (train || a.D != S::D || a.DIN != S::DIN || a.L != S::NH + 1 || a.act != S::ACT || a.sched || a.NG != S::NG || a.n_chunks != S::NCHUNK || a.l1rev) return ZK_EINVAL;
  for (int l = 0; l <= S::NH; ++l)
    if (!(a.wdescale[l] > 0.f) || !(a.wdescale[l] < __builtin_inff())) return ZK_EINVAL;  // the stream's per-layer scales must come with it
  a.n_tiles = (a.N + 16 * S::WAVES - 1) / (16 * S::WAVES);
  a.xs = ((S::D + 3) / 4) * 4 + 4;
  const bool term = a.base_loc != nullptr;  // terminal launch of a log_prob: y is not written
  if (term && (!a.base_scale || !a.ladj || a.bin_out || a.knots_out || !ArLds::base_fits(S::NG * 4 * Uni::FPL, S::D))) return ZK_EINVAL;
  const bool vec_ok = (S::D % 4 == 0) && (term || ((a.ldy % 4 == 0) && ((uintptr_t)a.y % 16 == 0)));
  if (S::XLDS != 0 && !vec_ok) return ZK_EINVAL;
  a.xlds = S::XLDS;
  const int lds = ArLds::bytes(S::NR * S::CH * AR_TF, a.bias_floats, S::XLDS ? S::WAVES : 0, a.xs);
  if (lds > 160 * 1024) return ZK_EINVAL;
  const void* fn = nullptr;
  if ((a.bin_out != nullptr) != (a.knots_out != nullptr)) return ZK_EINVAL;
  if (term) {
    fn = (const void*)arht_kernel<S, Uni>;
  } else if (a.bin_out) {
    if constexpr (Uni::NKNOT > 1) fn = (const void*)arh_kernel<S, Uni, true>;  // (the diagnostic twin exists for the spline maps only)
  } else {
    fn = (const void*)arh_kernel<S, Uni, false>;
  }
  if (!fn) return ZK_EINVAL;
  return ar_launch_dyn_lds(fn, 256, 64 * S::WAVES, lds, a, stream);
}

// ---- the FLOW launch: a workgroup carries its row tile through ALL T transforms of a composed autoregressive flow --------------------------------
// The transforms share one Shape (the same conditioner architecture; their feature orders and weights differ).  What differs per transform comes
// from the flow's own device buffers (zk_ar_common.h: ArhFlow; zuko_amd/fused.py: FusedFlow):
//   stream    (ArArgs::stream) the T transforms' streams back to back, S::NCHUNK whole chunks each: ONE ring over T NCHUNK chunks, whose look-ahead
//             crosses a transform boundary like any chunk boundary
//   bias      T bias images, bias_stride floats apart (whole 1 KiB pieces).  Two LDS buffers: a pass reads one while the ring requests the next
//             transform's into the other (ArhRing4::bias_request)
//   featmap   the n_fmaps DISTINCT feature maps of the flow (a flow that alternates two feature orders has two), all resident in LDS
//   table     per transform 8 words: the four descale factors of its stream (float), the index of its feature map (int), whether its first layer
//             follows the Shape's alternative in pairs (int; S::FLOW_ALT, S::B_IP_ALT: a flow that alternates two feature orders has two first-layer
//             patterns and nothing else that differs — one pass body serves both but for the 24-block first layer), 2 unused
// x is read and y, ladj (or, term, the log-density) are written once per tile; between two transforms the rows stay in the LDS row tile and the running
// log-derivative in a register.  Every transform's arithmetic is arh_pass's: the results are bitwise those of T launches of arh_kernel / arht_kernel.
template <class S, typename Uni> __device__ __forceinline__ void arhf_body(const ArArgs& a, const ArhFlow& f) {
  typedef ArhRing4<S::WAVES, S::CH, S::IMAGES, S::BPOS, true> Ring;
  static_assert(S::WAVES == 8 && S::NR == 4 && S::TMAX <= 16 && S::TMAX % 2 == 0 && S::OCC == 2 && S::NCHUNK >= 2, "flow kernel: the four-slot two-part geometry, two chunks or more per pass");
  constexpr int NT = Uni::NT, FPL = Uni::FPL, WAVES = S::WAVES, NG = S::NG, NFM = NG * 4 * FPL;
  static_assert(S::IMAGES == S::LAST_BASE + 2 * S::GOFF[NG] * NT && (S::IMAGES + S::CH - 1) / S::CH == S::NCHUNK, "stream length");
  const ArLane ln;
  const int tid = ln.tid, lane = ln.lane, wave = ln.wave, j = ln.j, q = ln.q;

  Ring ring;
  ring.start(ars_lds, a.stream, f.T * a.n_chunks, wave, lane);
  auto x_request = [&](int64_t tile, f32x4 (&xv)[S::NIT]) ARS_ALWAYS_INLINE {  // (arh_body's)
    const int64_t n = tile * (16 * WAVES) + wave * 16 + j;
    const float* row = a.x + (n < a.N ? n : a.N - 1) * a.ldx;
#pragma unroll
    for (int it = 0; it < S::NIT; ++it) {
      const int col = it * 16 + 4 * q;
      xv[it] = *reinterpret_cast<const f32x4*>(row + ((it + 1) * 16 <= S::DIN || col < S::DIN ? col : S::DIN - 4));
    }
  };
  f32x4 xnext[S::NIT];
  x_request(blockIdx.x, xnext);

  float* const bias_lds = ars_lds + S::NR * S::CH * AR_TF;  // two buffers of bias_stride floats
  int* const fmap_lds = ArLds::fmap(bias_lds, 2 * f.bias_stride);
  float* const xr = ArLds::row(fmap_lds, wave, j, a.xs);
  float* const base = ArLds::base(fmap_lds, f.n_fmaps * NFM);
  if (f.term) ArLds::stage_base<64 * WAVES>(a, tid, base, S::D);
  for (int i = tid; i < a.bias_floats; i += 64 * WAVES) bias_lds[i] = f.bias[i];  // the first transform's image; the others arrive through the ring
  for (int i = tid; i < f.n_fmaps * NFM; i += 64 * WAVES) fmap_lds[i] = f.featmap[i];
  __syncthreads();
  ring.bias_n = f.bias_stride / 256;
  const __attribute__((address_space(4))) float* const table = (const __attribute__((address_space(4))) float*)f.table;  // (uniform reads: scalar loads)

  int buf = 0;  // the bias buffer the pass in progress reads
  for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    ar_rows_in<S::D>(xr, q, xnext);
    float total = 0.f;
#pragma unroll 1
    for (int t = 0; t < f.T; ++t) {
      float wd[4];
#pragma unroll
      for (int l = 0; l < 4; ++l) wd[l] = table[t * 8 + l];
      const int fm = __builtin_bit_cast(int, table[t * 8 + 4]);
      const bool alt = __builtin_bit_cast(int, table[t * 8 + 5]) != 0;
      const int tn = t + 1 == f.T ? 0 : t + 1;
      ring.bias_src = reinterpret_cast<const char*>(f.bias + (size_t)tn * f.bias_stride);
      ring.bias_dst = reinterpret_cast<char*>(bias_lds + (buf ^ 1) * f.bias_stride);
      const ArFids<NG, FPL, (NG * FPL <= 32)> fids(fmap_lds + fm * NFM, q);
      arh_pass<S, Uni, false, false, true>(a, ring, x_request, xnext, bias_lds + buf * f.bias_stride, fids, xr, base, ln, tile, wd, t == 0, t + 1 == f.T, f.term != 0, total, alt);
      buf ^= 1;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // look-ahead DMAs must land before the LDS is released
}

template <class S, typename Uni> __global__ __launch_bounds__(64 * S::WAVES, S::OCC) void arhf_kernel(ArArgs a, ArhFlow f) { arhf_body<S, Uni>(a, f); }

// Launcher of the flow kernel (the entry point zk_arhf_launch of a unit of its own: zuko_amd/static_ar.py, ARHF).  A shape the kernel is not built for — three ring slots, rows not
// staged in LDS, context columns, a single chunk per pass — declines: the caller keeps the T launches.
template <class S, typename Uni> static int arhf_launch(const ArArgs* in, const ArhFlow* fin, int abi, int args_bytes, int flow_bytes, void* stream) {
  if (abi != ARS_ABI || args_bytes != (int)sizeof(ArArgs) || flow_bytes != (int)sizeof(ArhFlow)) return ZK_EINVAL;
  if constexpr (S::NR != 4 || !S::XLDS || S::DIN != S::D || S::D % 4 != 0 || S::NCHUNK < 2) {
    return ZK_EINVAL;
  } else {
    ArArgs a = *in;
    ArhFlow f = *fin;
    if (a.D != S::D || a.DIN != S::DIN || a.L != S::NH + 1 || a.act != S::ACT || a.sched || a.NG != S::NG || a.n_chunks != S::NCHUNK || a.l1rev) return ZK_EINVAL;
    if (f.T < 1 || f.T > 64 || f.n_fmaps < 1 || f.n_fmaps > f.T || f.bias_stride % 256 || f.bias_stride < a.bias_floats || !f.bias || !f.featmap || !f.table) return ZK_EINVAL;
    if (!a.x || !a.stream || !a.ladj || a.accumulate || a.bin_out || a.knots_out) return ZK_EINVAL;
    a.n_tiles = (a.N + 16 * S::WAVES - 1) / (16 * S::WAVES);
    a.xs = ((S::D + 3) / 4) * 4 + 4;
    f.term = a.base_loc != nullptr;
    if (f.term ? !a.base_scale : (!a.y || a.ldy % 4 != 0 || (uintptr_t)a.y % 16 != 0)) return ZK_EINVAL;
    if (f.n_fmaps * S::NG * 4 * Uni::FPL + (f.term ? 3 * S::D : 0) > ArLds::FMAP_WORDS) return ZK_EINVAL;
    a.xlds = 1;
    const int lds = ArLds::bytes(S::NR * S::CH * AR_TF, 2 * f.bias_stride, S::WAVES, a.xs);
    if (lds > 160 * 1024) return ZK_EINVAL;
    const void* fn = (const void*)arhf_kernel<S, Uni>;
    hipError_t e = grant_dyn_lds(fn, lds);
    if (e != hipSuccess) return (int)e;
    const unsigned grid = (unsigned)(a.n_tiles < 256 ? a.n_tiles : 256);
    void* kargs[] = {&a, &f};
    e = hipLaunchKernel(fn, dim3(grid), dim3(64 * S::WAVES), kargs, lds, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    return ZK_LAUNCH_CHECK();
  }
}

}  // namespace zk
