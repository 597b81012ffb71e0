// zuko_amd — wave-private staging of one contiguous run of values between HBM and LDS (the standalone univariate kernels, forward and backward).
//
// The LDS image keeps the run's alignment modulo 16 bytes: element i of the run sits at lds_aligned[shift + i] with
// shift = (address of the run / sizeof(T)) % (16 / sizeof(T)), so that after a scalar head every interior access is a full dwordx4 on both sides,
// followed by a scalar tail.  `lds_aligned` is 16-byte aligned and holds count + 2 * (16 / sizeof(T)) values.  The image belongs to ONE wavefront
// (`lane` = 0 .. 63): the callers order it against their own LDS accesses with s_waitcnt + wave_barrier, no workgroup barrier is involved.
#pragma once

#include "zk_common.h"

namespace zk {

// HBM -> LDS
template <typename T> __device__ __forceinline__ void stage_contiguous(const T* src, T* lds_aligned, int64_t count, int lane) {
  constexpr int VEC = 16 / sizeof(T);
  const int shift = (int)(((uintptr_t)src / sizeof(T)) % VEC);
  int head = shift ? (VEC - shift) : 0;
  if (head > count) head = (int)count;
  if (lane < head) lds_aligned[shift + lane] = src[lane];
  const int64_t body = (count - head) / VEC;
  const float4* vsrc = reinterpret_cast<const float4*>(src + head);
  float4* vdst = reinterpret_cast<float4*>(lds_aligned + shift + head);
  for (int64_t i = lane; i < body; i += ZK_WAVE) vdst[i] = vsrc[i];
  const int64_t done = head + body * VEC;
  const int tail = (int)(count - done);
  if (lane < tail) lds_aligned[shift + done + lane] = src[done + lane];
}

// LDS -> HBM, the mirror.  `shift` is the IMAGE's (that of the run it was staged from): `dst` must have the same alignment modulo 16 bytes
template <typename T> __device__ __forceinline__ void unstage_contiguous(const T* lds_aligned, int shift, T* dst, int64_t count, int lane) {
  constexpr int VEC = 16 / sizeof(T);
  int head = shift ? (VEC - shift) : 0;
  if (head > count) head = (int)count;
  if (lane < head) dst[lane] = lds_aligned[shift + lane];
  const int64_t body = (count - head) / VEC;
  const float4* vsrc = reinterpret_cast<const float4*>(lds_aligned + shift + head);
  float4* vdst = reinterpret_cast<float4*>(dst + head);
  for (int64_t i = lane; i < body; i += ZK_WAVE) vdst[i] = vsrc[i];
  const int64_t done = head + body * VEC;
  const int tail = (int)(count - done);
  if (lane < tail) dst[done + lane] = lds_aligned[shift + done + lane];
}

}  // namespace zk
