// What may stand between the matrix instructions of the two-part AR kernel's blocks (csrc/fused_ar_half_impl.h: arh_wait_block) when BOTH wavefronts
// of a SIMD issue matrix instructions and both carry the fillers?  Every wavefront runs the kernel's block form — two raw ds_read_b128 one block
// ahead, the counted wait, a dependent chain of three v_mfma_f32_16x16x32_f16 on one accumulator — with F = 0..3 fillers of ONE kind behind every
// matrix instruction.  Fillers are independent of each other and of the matrix instructions (own destinations, constant sources).
// Reported: shader cycles (s_memtime) per matrix instruction, per wavefront and per SIMD (the wavefront figure over the wavefronts a SIMD holds).
//
//   hipcc -O3 --offload-arch=gfx950 scripts/probes/gap_fill_probe.hip -o scripts/probes/gap_fill_probe && scripts/probes/gap_fill_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int UNROLL = 8;  // blocks per loop iteration (24 matrix instructions)
constexpr int NKIND = 9;
static const char* const KIND_NAME[NKIND] = {"v_fma_f32", "v_fma_mixlo_f16", "v_cndmask_b32", "v_max_f32", "v_exp_f32", "v_rcp_f32", "v_pk_mul_f32", "v_pk_add_f32", "v_pk_fma_f32"};

// one filler of each kind, destination D (t0..t8: one register, p0..p8: a pair)
#define FILL_0(D) "v_fma_f32 %[t" D "], %[x], %[y], %[t" D "]\n\t"
#define FILL_1(D) "v_fma_mixlo_f16 %[t" D "], %[x], %[y], %[x]\n\t"
#define FILL_2(D) "v_cndmask_b32 %[t" D "], %[x], %[y], %[m]\n\t"
#define FILL_3(D) "v_max_f32 %[t" D "], %[x], %[y]\n\t"
#define FILL_4(D) "v_exp_f32 %[t" D "], %[x]\n\t"
#define FILL_5(D) "v_rcp_f32 %[t" D "], %[x]\n\t"
#define FILL_6(D) "v_pk_mul_f32 %[p" D "], %[x2], %[y2]\n\t"
#define FILL_7(D) "v_pk_add_f32 %[p" D "], %[x2], %[y2]\n\t"
#define FILL_8(D) "v_pk_fma_f32 %[p" D "], %[x2], %[y2], %[p" D "]\n\t"
#define GAP_0(FILL, A, B, C) ""
#define GAP_1(FILL, A, B, C) FILL(A)
#define GAP_2(FILL, A, B, C) FILL(A) FILL(B)
#define GAP_3(FILL, A, B, C) FILL(A) FILL(B) FILL(C)
#define BLOCK(FILL, GAP)                                                                                                                            \
  asm volatile("v_mfma_f32_16x16x32_f16 %[c], %[al], %[bh], %[c]\n\t" GAP(FILL, "0", "1", "2")                                                      \
               "v_mfma_f32_16x16x32_f16 %[c], %[ah], %[bl], %[c]\n\t" GAP(FILL, "3", "4", "5")                                                      \
               "v_mfma_f32_16x16x32_f16 %[c], %[ah], %[bh], %[c]\n\t" GAP(FILL, "6", "7", "8")                                                      \
               : [c] "+v"(c), [t0] "+v"(t[0]), [t1] "+v"(t[1]), [t2] "+v"(t[2]), [t3] "+v"(t[3]), [t4] "+v"(t[4]), [t5] "+v"(t[5]), [t6] "+v"(t[6]), \
                 [t7] "+v"(t[7]), [t8] "+v"(t[8]), [p0] "+v"(p[0]), [p1] "+v"(p[1]), [p2] "+v"(p[2]), [p3] "+v"(p[3]), [p4] "+v"(p[4]),              \
                 [p5] "+v"(p[5]), [p6] "+v"(p[6]), [p7] "+v"(p[7]), [p8] "+v"(p[8])                                                                  \
               : [ah] "v"(a[cur][0]), [al] "v"(a[cur][1]), [bh] "v"(bh), [bl] "v"(bl), [x] "v"(x), [y] "v"(y), [x2] "v"(x2), [y2] "v"(y2), [m] "s"(m))
#define BLOCK_F(FILL)                        \
  if constexpr (F == 0) BLOCK(FILL, GAP_0);  \
  else if constexpr (F == 1) BLOCK(FILL, GAP_1); \
  else if constexpr (F == 2) BLOCK(FILL, GAP_2); \
  else BLOCK(FILL, GAP_3)

template <int KIND, int F> __global__ __launch_bounds__(512, 1) void probe(float* out, unsigned long long* ticks, int iters) {
  __shared__ float img[2 * 2 * 256];  // two blocks of two 1 KiB weight images
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < 2 * 2 * 256; i += blockDim.x) img[i] = 0.f;
  __syncthreads();
  const unsigned addr = (unsigned)(size_t)((__attribute__((address_space(3))) float*)img) + (unsigned)lane * 16;
  f16x8 bh, bl;
  for (int e = 0; e < 8; ++e) { bh[e] = (_Float16)(1.f + e); bl[e] = (_Float16)(0.001f * e); }
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  float t[9];
  f32x2 p[9];
  for (int i = 0; i < 9; ++i) { t[i] = 0.5f + i; p[i] = f32x2{0.25f + i, 1.f}; }
  const float x = 0.75f + lane * 0.001f, y = 1.0009765625f;
  const f32x2 x2 = {x, y}, y2 = {y, x};
  const unsigned long long m = 0x5555555555555555ull;
  f32x4 a[2][2];
  asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024" : "=v"(a[0][0]), "=v"(a[0][1]) : "v"(addr));
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int cur = u & 1, nx = cur ^ 1;
      if (nx) asm volatile("ds_read_b128 %0, %2 offset:2048\n\tds_read_b128 %1, %2 offset:3072" : "=v"(a[1][0]), "=v"(a[1][1]) : "v"(addr));
      else asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024" : "=v"(a[0][0]), "=v"(a[0][1]) : "v"(addr));
      __builtin_amdgcn_s_waitcnt(0xC07F | (2 << 8));  // lgkmcnt(2), as the compiler's instruction (arh_wait_block: an asm wait draws one s_nop per block)
      if constexpr (KIND == 0) { BLOCK_F(FILL_0); }
      else if constexpr (KIND == 1) { BLOCK_F(FILL_1); }
      else if constexpr (KIND == 2) { BLOCK_F(FILL_2); }
      else if constexpr (KIND == 3) { BLOCK_F(FILL_3); }
      else if constexpr (KIND == 4) { BLOCK_F(FILL_4); }
      else if constexpr (KIND == 5) { BLOCK_F(FILL_5); }
      else if constexpr (KIND == 6) { BLOCK_F(FILL_6); }
      else if constexpr (KIND == 7) { BLOCK_F(FILL_7); }
      else { BLOCK_F(FILL_8); }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[1][0]), "+v"(a[1][1]));
  asm volatile("s_nop 15" : "+v"(c));
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  float s = c[0] + c[1] + c[2] + c[3] + a[0][0][0] + a[1][1][0];
  for (int i = 0; i < 9; ++i) s += t[i] + p[i][0] + p[i][1];
  out[blockIdx.x * 512 + threadIdx.x] = s;
  if (lane == 0) ticks[blockIdx.x * 8 + (threadIdx.x >> 6)] = t1 - t0;
}

constexpr int BLOCKS = 256, ITERS = 2000;
#define CHECK(X) do { if ((X) != hipSuccess) { printf("%s failed\n", #X); exit(1); } } while (0)

struct Row { double mean, worst, ms; };

template <int KIND, int F> Row run(float* out, unsigned long long* ticks, int threads) {
  const int waves = threads / 64;
  std::vector<unsigned long long> h(BLOCKS * 8);
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  float ms = 0.f;
  for (int rep = 0; rep < 2; ++rep) {  // (the first run warms the clocks and the instruction cache)
    CHECK(hipEventRecord(e0));
    probe<KIND, F><<<BLOCKS, threads>>>(out, ticks, ITERS);
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    CHECK(hipEventElapsedTime(&ms, e0, e1));
  }
  CHECK(hipMemcpy(h.data(), ticks, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
  CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
  const double n = double(ITERS) * UNROLL * 3;
  double sum = 0, worst = 0;
  for (int b = 0; b < BLOCKS; ++b)
    for (int w = 0; w < waves; ++w) { sum += h[b * 8 + w] / n; worst = std::max(worst, h[b * 8 + w] / n); }
  return {sum / (BLOCKS * waves), worst, ms};
}

template <int KIND> void kind(float* out, unsigned long long* ticks, int threads) {
  const Row r[4] = {run<KIND, 0>(out, ticks, threads), run<KIND, 1>(out, ticks, threads), run<KIND, 2>(out, ticks, threads), run<KIND, 3>(out, ticks, threads)};
  const int per_simd = threads / 256;
  printf("%-16s", KIND_NAME[KIND]);
  for (int f = 0; f < 4; ++f) printf("  %6.2f (%6.2f)", r[f].mean / per_simd, r[f].mean);
  printf("   +%5.2f +%5.2f +%5.2f   %6.3f ms\n", (r[1].mean - r[0].mean) / per_simd, (r[2].mean - r[0].mean) / per_simd, (r[3].mean - r[0].mean) / per_simd, r[3].ms);
}

void table(float* out, unsigned long long* ticks, int threads) {
  printf("\n%d wavefront(s) per SIMD, every wavefront: 2 ds_read_b128, s_waitcnt lgkmcnt(2), 3 dependent v_mfma_f32_16x16x32_f16, F fillers behind each\n", threads / 256);
  printf("cycles per matrix instruction per SIMD (per wavefront): F = 0, 1, 2, 3; then the SIMD's cost of F = 1, 2, 3 over F = 0; kernel time at F = 3\n");
  kind<0>(out, ticks, threads); kind<1>(out, ticks, threads); kind<2>(out, ticks, threads); kind<3>(out, ticks, threads); kind<4>(out, ticks, threads);
  kind<5>(out, ticks, threads); kind<6>(out, ticks, threads); kind<7>(out, ticks, threads); kind<8>(out, ticks, threads);
}

int main() {
  float* out;
  unsigned long long* ticks;
  CHECK(hipMalloc(&out, BLOCKS * 512 * sizeof(float)));
  CHECK(hipMalloc(&ticks, BLOCKS * 8 * sizeof(unsigned long long)));
  table(out, ticks, 512);
  table(out, ticks, 256);
  CHECK(hipFree(out)); CHECK(hipFree(ticks));
  return 0;
}
