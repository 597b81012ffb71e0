// zuko_amd — Gaussian mixture density and its adjoint for gfx950 (zk_gmm_log_prob / zk_gmm_backward, include/zuko_amd.h).
//
// One row of phi is  logits[K] | loc[K, D] | diag[Lc, Dd] | tril[Lc, D(D-1)/2]  (Lc = 1 if tied else K; Dd = 1 for spherical, else D;
// tril only for full covariance, the strict lower triangle row by row).  L_ii = exp(diag_i) + epsilon, L_ij = tril (i > j).
//
// Execution model.  A block is ONE wave of 64 lanes and owns R consecutive rows (R = 64 where the tile fits 64 KiB of LDS,
// else the next power of two that does: gmm_rows_per_block).  Lane r does all the arithmetic of row r, in a fixed order, so a row's result
// depends on its own x, phi row and g only.  phi never reaches the lanes directly: the wave copies one SEGMENT of every row of the tile (the
// logits; then per component loc_k | diag_k; then a window of whole rows of tril_k, at most GMM_CHUNK elements) into an LDS tile
// stage[R][P] with consecutive lanes on consecutive addresses, 16 bytes per lane where the address allows (gmm_load_seg: scalar head up to
// the next 16-byte boundary, vector body, scalar tail: total is often odd, so rows are 4-byte aligned in general).  P is odd: lane r reading
// stage[r * P + e] hits 32 (64) distinct banks.  x, the substitution vector z, its adjoint a and the per-component terms live in LDS as
// [index][R] columns (lane-private, conflict-free): there is no per-thread array, hence no scratch memory, for any D.
// Gradients leave the same way: the lanes write their row's values into the stage tile, the wave stores the segment coalesced
// (gmm_store_seg; for tied covariance it adds component k > 0 to what component k - 1 left, the same lane each time: no atomics).
// Shared row (ld_phi = 0): the block adds the tile's rows in row order into its own partial [total] vector in `work` (tiles of one block in
// tile order), and gmm_reduce_partials adds the partials in block order.
//
// Built with -ffp-contract=off: every product and sum rounds once, in the order written here.

#include "../../include/zuko_amd.h"
#include "zk_common.h"

namespace zk {

constexpr int GMM_THREADS = 64;
constexpr int GMM_CHUNK = 128;            // elements of tril staged at once; >= D - 1 = 63, the longest row
constexpr int GMM_LDS_BYTES = 64 * 1024;  // per block: no opt-in to large LDS needed
constexpr int GMM_FULL = 0, GMM_DIAGONAL = 1, GMM_SPHERICAL = 2;

struct GmmShape {
  int D, K, cov, tied, Dd, Lc, T;
  int off_loc, off_diag, off_tril, total;
  int H, CW, P;  // head (loc | diag) and tril window of the stage tile, its pitch
};

static bool gmm_shape(int D, int K, int cov, int tied, GmmShape* s) {
  if (D < 1 || D > 64 || K < 1 || K > 64 || cov < 0 || cov > 2 || (tied != 0 && tied != 1)) return false;
  s->D = D, s->K = K, s->cov = cov, s->tied = tied;
  s->Dd = cov == GMM_SPHERICAL ? 1 : D;
  s->Lc = tied ? 1 : K;
  s->T = cov == GMM_FULL ? D * (D - 1) / 2 : 0;
  s->off_loc = K;
  s->off_diag = K + K * D;
  s->off_tril = s->off_diag + s->Lc * s->Dd;
  s->total = s->off_tril + s->Lc * s->T;
  s->H = D + s->Dd;
  s->CW = s->T < GMM_CHUNK ? s->T : GMM_CHUNK;
  const int w = s->H + s->CW > K ? s->H + s->CW : K;
  s->P = w | 1;
  return true;
}

// LDS elements per row: x, z, L_ii, a, gx as [D] columns, t and w as [K] columns, the stage row.  One figure for both kernels, so that one
// geometry answers for both.
static int gmm_row_elems(const GmmShape& s) { return 5 * s.D + 2 * s.K + s.P; }

static int gmm_rows_per_block(const GmmShape& s, int dtype) {
  const int esz = dtype == ZK_DTYPE_F64 ? 8 : 4;
  int R = GMM_THREADS;
  while (R > 1 && R * gmm_row_elems(s) * esz > GMM_LDS_BYTES) R >>= 1;
  return R;
}

// blocks of the shared-row backward (= partial vectors in `work`): at most 1024, fewer for long rows (<= 64 MiB of float32 partials)
static int gmm_partial_blocks(const GmmShape& s, long long ntiles) {
  long long cap = (1ll << 24) / s.total;
  cap = cap < 64 ? 64 : (cap > 1024 ? 1024 : cap);
  return (int)(ntiles < cap ? ntiles : cap);
}

template <typename T> struct GmmArgs {
  const T* x;
  const T* phi;
  const T* g;
  T* out;
  T* gphi;
  T* gx;
  T* work;
  long long N, ldx, ld_phi, ld_gphi, ld_gx;
  GmmShape s;
  int R;
  T eps, dlog2pi;
};

template <typename T> struct GmmVec;
template <> struct GmmVec<float> { typedef float4 type; static constexpr int n = 4; };
template <> struct GmmVec<double> { typedef double2 type; static constexpr int n = 2; };

__device__ __forceinline__ void gmm_unpack(const float4& v, float* d) { d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w; }
__device__ __forceinline__ void gmm_unpack(const double2& v, double* d) { d[0] = v.x, d[1] = v.y; }
__device__ __forceinline__ float4 gmm_pack(const float* d) { return make_float4(d[0], d[1], d[2], d[3]); }
__device__ __forceinline__ double2 gmm_pack(const double* d) { return make_double2(d[0], d[1]); }
__device__ __forceinline__ float4 gmm_add(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ double2 gmm_add(const double2& a, const double2& b) { return make_double2(a.x + b.x, a.y + b.y); }

// lanes that share one row's segment: a power of two, >= 4 (the scalar head and tail are < 4 elements), one 16-byte piece per lane where possible
__device__ __forceinline__ int gmm_group(int len, int vec) {
  const int pieces = (len + vec - 1) / vec;
  int G = 4;
  while (G < GMM_THREADS && G < pieces) G <<= 1;
  return G;
}

// stage[r * P + dst + e] = base[(row0 + r) * ld + off + e], e < len, r < nrows
template <typename T>
__device__ __forceinline__ void gmm_load_seg(const T* __restrict__ base, long long ld, long long row0, int nrows, int off, int len, T* stage, int P, int dst) {
  typedef typename GmmVec<T>::type V;
  constexpr int VN = GmmVec<T>::n;
  const int G = gmm_group(len, VN), g = threadIdx.x & (G - 1), per = GMM_THREADS / G;
  for (int r = threadIdx.x / G; r < nrows; r += per) {
    const T* p = base + (row0 + r) * ld + off;
    T* d = stage + r * P + dst;
    int head = (int)((16 - ((uintptr_t)p & 15)) & 15) / (int)sizeof(T);
    head = head < len ? head : len;
    if (g < head) d[g] = p[g];
    const int nvec = (len - head) / VN;
    for (int v = g; v < nvec; v += G) {
      const V q = *reinterpret_cast<const V*>(p + head + v * VN);
      gmm_unpack(q, d + head + v * VN);
    }
    const int t0 = head + nvec * VN;
    if (g < len - t0) d[t0 + g] = p[t0 + g];
  }
}

// base[(row0 + r) * ld + off + e] (+)= stage[r * P + src + e]; the lane that owns an element is the same for every call with this len and address
template <typename T>
__device__ __forceinline__ void gmm_store_seg(T* __restrict__ base, long long ld, long long row0, int nrows, int off, int len, const T* stage, int P, int src, bool add) {
  typedef typename GmmVec<T>::type V;
  constexpr int VN = GmmVec<T>::n;
  const int G = gmm_group(len, VN), g = threadIdx.x & (G - 1), per = GMM_THREADS / G;
  for (int r = threadIdx.x / G; r < nrows; r += per) {
    T* p = base + (row0 + r) * ld + off;
    const T* s = stage + r * P + src;
    int head = (int)((16 - ((uintptr_t)p & 15)) & 15) / (int)sizeof(T);
    head = head < len ? head : len;
    if (g < head) p[g] = add ? p[g] + s[g] : s[g];
    const int nvec = (len - head) / VN;
    for (int v = g; v < nvec; v += G) {
      V* q = reinterpret_cast<V*>(p + head + v * VN);
      V val = gmm_pack(s + head + v * VN);
      if (add) val = gmm_add(*q, val);
      *q = val;
    }
    const int t0 = head + nvec * VN;
    if (g < len - t0) p[t0 + g] = add ? p[t0 + g] + s[t0 + g] : s[t0 + g];
  }
}

// partial[off + e] (+)= sum over the tile's rows, r = 0, 1, ..., of stage[r * P + src + e]
template <typename T>
__device__ __forceinline__ void gmm_reduce_seg(T* __restrict__ partial, int nrows, int off, int len, const T* stage, int P, int src, bool add) {
  for (int e = threadIdx.x; e < len; e += GMM_THREADS) {
    T s = stage[src + e];
    for (int r = 1; r < nrows; ++r) s += stage[r * P + src + e];
    partial[off + e] = add ? partial[off + e] + s : s;
  }
}

__device__ __forceinline__ int gmm_tri(int i) { return i * (i - 1) / 2; }  // offset of row i of the strict lower triangle

extern __shared__ __attribute__((aligned(16))) unsigned char gmm_lds[];

template <typename T> struct GmmLds {
  T *xs, *zs, *Ls, *ts, *stage, *as, *gxs, *ws;
  __device__ __forceinline__ GmmLds(const GmmShape& s, int R) {
    T* p = reinterpret_cast<T*>(gmm_lds);
    xs = p, p += s.D * R;
    zs = p, p += s.D * R;
    Ls = p, p += s.D * R;
    as = p, p += s.D * R;
    gxs = p, p += s.D * R;
    ts = p, p += s.K * R;
    ws = p, p += s.K * R;
    stage = p;
  }
};

// Component k of the tile: stages loc_k | diag_k (left in stage[0 .. H) of every row) and the rows of tril_k window by window; leaves
// z_k = L_k^{-1} (x - loc_k) in zs and L_ii in Ls; returns log N(x | loc_k, L_k L_k^T) in the valid lanes.  Every lane of the block calls it.
template <typename T>
__device__ __forceinline__ T gmm_component(const GmmArgs<T>& a, const GmmLds<T>& m, int k, long long row0, int nrows) {
  const GmmShape& s = a.s;
  const int D = s.D, R = a.R, P = s.P, lane = threadIdx.x, kc = s.tied ? 0 : k;
  const bool valid = lane < nrows;
  T* st = m.stage + lane * P;
  __syncthreads();  // the stage tile is free (previous component, previous segment)
  gmm_load_seg(a.phi, a.ld_phi, row0, nrows, s.off_loc + k * D, D, m.stage, P, 0);
  gmm_load_seg(a.phi, a.ld_phi, row0, nrows, s.off_diag + kc * s.Dd, s.Dd, m.stage, P, D);
  __syncthreads();
  T logdet = T(0);
  if (valid) {
    T L = T(0), lL = T(0);
    for (int i = 0; i < D; ++i) {
      if (i == 0 || s.Dd > 1) {
        L = t_exp(st[D + i]) + a.eps;
        lL = t_log(L);
        m.Ls[i * R + lane] = L;
      }
      logdet += lL;
      const T d = m.xs[i * R + lane] - st[i];
      m.zs[i * R + lane] = (s.cov != GMM_FULL || i == 0) ? d / L : d;
    }
  }
  if (s.cov == GMM_FULL) {
    for (int i0 = 1; i0 < D;) {
      int i1 = i0 + 1;
      while (i1 < D && gmm_tri(i1 + 1) - gmm_tri(i0) <= s.CW) ++i1;
      __syncthreads();
      gmm_load_seg(a.phi, a.ld_phi, row0, nrows, s.off_tril + kc * s.T + gmm_tri(i0), gmm_tri(i1) - gmm_tri(i0), m.stage, P, s.H);
      __syncthreads();
      if (valid) {
        for (int i = i0; i < i1; ++i) {
          const T* Lrow = st + s.H + gmm_tri(i) - gmm_tri(i0);
          T acc = T(0);
          for (int j = 0; j < i; ++j) acc += Lrow[j] * m.zs[j * R + lane];
          m.zs[i * R + lane] = (m.zs[i * R + lane] - acc) / m.Ls[i * R + lane];
        }
      }
      i0 = i1;
    }
  }
  T q = T(0);
  if (valid)
    for (int i = 0; i < D; ++i) {
      const T z = m.zs[i * R + lane];
      q += z * z;
    }
  return T(-0.5) * (a.dlog2pi + q) - logdet;
}

template <typename T, bool BWD> __global__ __launch_bounds__(GMM_THREADS) void gmm_kernel(GmmArgs<T> a) {
  const GmmShape& s = a.s;
  const GmmLds<T> m(s, a.R);
  const int D = s.D, K = s.K, R = a.R, P = s.P, lane = threadIdx.x;
  const long long ntiles = (a.N + R - 1) / R;
  const bool shared = BWD && a.ld_phi == 0;
  T* partial = (shared && a.gphi) ? a.work + (long long)blockIdx.x * s.total : nullptr;
  T* st = m.stage + lane * P;
  const T INF = (T)__builtin_inf();
  bool again = false;  // shared row: this block's partial already holds a tile
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long row0 = tile * R;
    const int nrows = (int)(a.N - row0 < R ? a.N - row0 : R);
    const bool valid = lane < nrows;
    __syncthreads();
    for (int e = lane; e < nrows * D; e += GMM_THREADS) {
      const int r = e / D, c = e - r * D;
      m.xs[c * R + r] = a.x[(row0 + r) * a.ldx + c];
    }
    gmm_load_seg(a.phi, a.ld_phi, row0, nrows, 0, K, m.stage, P, 0);
    __syncthreads();
    if (valid) {  // log_softmax(logits) = (l - max) - log(sum exp(l - max))
      T mx = -INF, sum = T(0);
      for (int k = 0; k < K; ++k) mx = st[k] > mx ? st[k] : mx;
      for (int k = 0; k < K; ++k) sum += t_exp(st[k] - mx);
      const T ls = t_log(sum);
      for (int k = 0; k < K; ++k) {
        const T lw = (st[k] - mx) - ls;
        m.ts[k * R + lane] = lw;
        if (BWD) m.ws[k * R + lane] = lw;
      }
    }
    for (int k = 0; k < K; ++k) {
      const T logn = gmm_component(a, m, k, row0, nrows);
      if (valid) m.ts[k * R + lane] += logn;
    }
    // logsumexp: the maximum is subtracted unless it is infinite (all terms -inf give log(0) = -inf, not exp(-inf + inf))
    T mx = -INF, sum = T(0);
    if (valid) {
      for (int k = 0; k < K; ++k) mx = m.ts[k * R + lane] > mx ? m.ts[k * R + lane] : mx;
      if (mx == INF || mx == -INF) mx = T(0);
      for (int k = 0; k < K; ++k) sum += t_exp(m.ts[k * R + lane] - mx);
    }
    if (!BWD) {
      if (valid) a.out[row0 + lane] = t_log(sum) + mx;
      continue;
    }
    if (valid) {
      const T g = a.g[row0 + lane];
      for (int k = 0; k < K; ++k) {
        const T r = t_exp(m.ts[k * R + lane] - mx) / sum;
        const T w = t_exp(m.ws[k * R + lane]);
        m.ts[k * R + lane] = g * r;        // g r_k
        m.ws[k * R + lane] = g * (r - w);  // d / d logits_k
      }
      for (int i = 0; i < D; ++i) m.gxs[i * R + lane] = T(0);
    }
    for (int k = 0; k < K; ++k) {
      const int kc = s.tied ? 0 : k;
      const bool add_cov = (s.tied && k > 0) || again;
      gmm_component(a, m, k, row0, nrows);  // z_k, L_ii again; loc_k | diag_k in stage[0 .. H)
      const T gr = valid ? m.ts[k * R + lane] : T(0);
      if (valid) {
        if (s.cov == GMM_FULL)
          for (int i = 0; i < D; ++i) m.as[i * R + lane] = m.zs[i * R + lane];
        else
          for (int i = 0; i < D; ++i) m.as[i * R + lane] = m.zs[i * R + lane] / m.Ls[(s.Dd > 1 ? i : 0) * R + lane];
      }
      if (s.cov == GMM_FULL) {
        // a = L^{-T} z from the last row up: a_j = acc_j / L_jj, then acc_i -= L_ji a_j for i < j; row j of tril turns into its gradient in place
        for (int i1 = D; i1 > 1;) {
          int i0 = i1 - 1;
          while (i0 > 1 && gmm_tri(i1) - gmm_tri(i0 - 1) <= s.CW) --i0;
          const int off = s.off_tril + kc * s.T + gmm_tri(i0), len = gmm_tri(i1) - gmm_tri(i0);
          __syncthreads();
          gmm_load_seg(a.phi, a.ld_phi, row0, nrows, off, len, m.stage, P, s.H);
          __syncthreads();
          if (valid) {
            for (int j = i1 - 1; j >= i0; --j) {
              T* Lrow = st + s.H + gmm_tri(j) - gmm_tri(i0);
              const T aj = m.as[j * R + lane] / m.Ls[j * R + lane];
              m.as[j * R + lane] = aj;
              const T gaj = gr * aj;
              for (int i = 0; i < j; ++i) {
                m.as[i * R + lane] -= Lrow[i] * aj;
                Lrow[i] = gaj * m.zs[i * R + lane];
              }
            }
          }
          if (a.gphi) {
            __syncthreads();
            if (shared) gmm_reduce_seg(partial, nrows, off, len, m.stage, P, s.H, add_cov);
            else gmm_store_seg(a.gphi, a.ld_gphi, row0, nrows, off, len, m.stage, P, s.H, add_cov);
          }
          i1 = i0;
        }
        if (valid) m.as[lane] = m.as[lane] / m.Ls[lane];
      }
      if (valid) {
        T gsum = T(0);
        for (int i = 0; i < D; ++i) {
          const int dd = s.Dd > 1 ? i : 0;
          const T ai = m.as[i * R + lane], zi = m.zs[i * R + lane], Li = m.Ls[dd * R + lane];
          const T gl = gr * ai;
          const T gd = gr * (ai * zi - T(1) / Li) * t_exp(st[D + dd]);
          st[i] = gl;
          m.gxs[i * R + lane] += gl;
          if (s.Dd > 1) st[D + i] = gd;
          else gsum += gd;
        }
        if (s.Dd == 1) st[D] = gsum;
      }
      if (a.gphi) {
        __syncthreads();
        if (shared) {
          gmm_reduce_seg(partial, nrows, s.off_loc + k * D, D, m.stage, P, 0, again);
          gmm_reduce_seg(partial, nrows, s.off_diag + kc * s.Dd, s.Dd, m.stage, P, D, add_cov);
        } else {
          gmm_store_seg(a.gphi, a.ld_gphi, row0, nrows, s.off_loc + k * D, D, m.stage, P, 0, false);
          gmm_store_seg(a.gphi, a.ld_gphi, row0, nrows, s.off_diag + kc * s.Dd, s.Dd, m.stage, P, D, add_cov);
        }
      }
    }
    __syncthreads();
    if (a.gphi) {
      if (valid)
        for (int k = 0; k < K; ++k) st[k] = m.ws[k * R + lane];
      __syncthreads();
      if (shared) gmm_reduce_seg(partial, nrows, 0, K, m.stage, P, 0, again);
      else gmm_store_seg(a.gphi, a.ld_gphi, row0, nrows, 0, K, m.stage, P, 0, false);
    }
    if (a.gx)
      for (int e = lane; e < nrows * D; e += GMM_THREADS) {
        const int r = e / D, c = e - r * D;
        a.gx[(row0 + r) * a.ld_gx + c] = -m.gxs[c * R + r];
      }
    again = shared;
  }
}

// gphi[e] = sum over the blocks' partial vectors, b = 0, 1, ...
template <typename T> __global__ __launch_bounds__(256) void gmm_reduce_partials(const T* __restrict__ work, int nblocks, int total, T* __restrict__ gphi) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  T s = work[e];
  for (int b = 1; b < nblocks; ++b) s += work[(long long)b * total + e];
  gphi[e] = s;
}

static bool gmm_check(const zk_gmm_args_v1* p, bool bwd, GmmShape* s) {
  if (!p || p->struct_size != sizeof(zk_gmm_args_v1) || p->version != 1 || p->reserved != 0) return false;
  if (p->dtype != ZK_DTYPE_F32 && p->dtype != ZK_DTYPE_F64) return false;
  if (!gmm_shape(p->D, p->K, p->covariance, p->tied, s)) return false;
  if (p->N < 1 || !p->x || !p->phi || p->ldx < p->D) return false;
  if (p->ld_phi != 0 && p->ld_phi < s->total) return false;
  if (!bwd) return p->out != nullptr;
  if (!p->g || (!p->gphi && !p->gx)) return false;
  if (p->gphi && (p->ld_phi == 0 ? p->work == nullptr : p->ld_gphi < s->total)) return false;
  if (p->gx && p->ld_gx < p->D) return false;
  return true;
}

template <typename T, bool BWD> static int gmm_launch_t(const zk_gmm_args_v1* p, const GmmShape& s, void* stream) {
  GmmArgs<T> a;
  a.x = (const T*)p->x, a.phi = (const T*)p->phi, a.g = (const T*)p->g;
  a.out = (T*)p->out, a.gphi = (T*)p->gphi, a.gx = (T*)p->gx, a.work = (T*)p->work;
  a.N = p->N, a.ldx = p->ldx, a.ld_phi = p->ld_phi, a.ld_gphi = p->ld_gphi, a.ld_gx = p->ld_gx;
  a.s = s;
  a.R = gmm_rows_per_block(s, p->dtype);
  a.eps = (T)p->epsilon;
  a.dlog2pi = (T)((double)s.D * 1.8378770664093454836);  // D log(2 pi)
  const long long ntiles = (a.N + a.R - 1) / a.R;
  const bool shared = BWD && a.ld_phi == 0 && a.gphi;
  const long long grid = shared ? gmm_partial_blocks(s, ntiles) : (ntiles < (1ll << 30) ? ntiles : (1ll << 30));
  const size_t lds = (size_t)a.R * gmm_row_elems(s) * sizeof(T);
  hipLaunchKernelGGL((gmm_kernel<T, BWD>), dim3((unsigned)grid), dim3(GMM_THREADS), lds, (hipStream_t)stream, a);
  int err = ZK_LAUNCH_CHECK();
  if (err == 0 && shared) {
    hipLaunchKernelGGL((gmm_reduce_partials<T>), dim3((s.total + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const T*)a.work, (int)grid, s.total, a.gphi);
    err = ZK_LAUNCH_CHECK();
  }
  return err;
}

template <bool BWD> static int gmm_launch(const zk_gmm_args_v1* p, void* stream) {
  GmmShape s;
  if (!gmm_check(p, BWD, &s)) return ZK_EINVAL;
  return p->dtype == ZK_DTYPE_F64 ? gmm_launch_t<double, BWD>(p, s, stream) : gmm_launch_t<float, BWD>(p, s, stream);
}

}  // namespace zk

extern "C" int zk_gmm_log_prob(const zk_gmm_args_v1* args, void* stream) { return zk::gmm_launch<false>(args, stream); }
extern "C" int zk_gmm_backward(const zk_gmm_args_v1* args, void* stream) { return zk::gmm_launch<true>(args, stream); }
extern "C" int zk_gmm_total(int D, int K, int covariance, int tied) {
  zk::GmmShape s;
  return zk::gmm_shape(D, K, covariance, tied, &s) ? s.total : -1;
}
extern "C" int zk_gmm_launch_geometry(int dtype, int D, int K, int covariance, int tied, int* rows_per_block) {
  zk::GmmShape s;
  if ((dtype != ZK_DTYPE_F32 && dtype != ZK_DTYPE_F64) || !rows_per_block || !zk::gmm_shape(D, K, covariance, tied, &s)) return ZK_EINVAL;
  *rows_per_block = zk::gmm_rows_per_block(s, dtype);
  return 0;
}
extern "C" int zk_gmm_workspace_floats(int dtype, int64_t N, int D, int K, int covariance, int tied) {
  zk::GmmShape s;
  if ((dtype != ZK_DTYPE_F32 && dtype != ZK_DTYPE_F64) || N < 1 || !zk::gmm_shape(D, K, covariance, tied, &s)) return -1;
  const int R = zk::gmm_rows_per_block(s, dtype);
  return zk::gmm_partial_blocks(s, (N + R - 1) / R) * s.total;
}
