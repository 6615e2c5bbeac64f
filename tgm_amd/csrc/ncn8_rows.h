// What the k = 8 NCNPredictor forward (ncn8.hip) and its backward (ncn8_bwd.hip) share: the five int32 count rows of a pair -- their storage
// (LDS, or a region of global memory per resident workgroup), the two-hop walk that fills and clears them, K3[t, t] -- and the float64 decay
// weight.  One definition, so the backward's coefficients are the forward's, bit for bit.
#pragma once
#include "common.h"
#include "edge_csr.h"
#include "ncn_rows.h"

#include <atomic>

namespace tgmx {

constexpr int kNcn8Threads = 256;
constexpr int kNcn8Waves = kNcn8Threads / kWave;
constexpr int kNcn8Rows = 5;
// LDS: a CU has 160 KiB (163 840 bytes) and a workgroup may take all of it.  A workgroup takes 20 N bytes of rows (dynamic) beside 8 272
// bytes of static chunk list (s_id 1 KiB, s_cf 5 KiB, s_w 2 KiB, s_cnt, s_k3): 150 KiB + 8.1 KiB at the cap of 7680 ids.  Workgroups (of
// 4 waves) per CU: ONE for 3683 <= N <= 7680, 2 up to N = 3682, 3 up to 2317, 4 up to 1634, 5 at the N = 1000 of a small batch, 8 up to
// N = 610.  The example's batch (B = 200 pairs) has fewer workgroups than the 256 CUs, so one resident workgroup per CU is all it can use.
constexpr int kNcn8LdsMaxN = 7680;
constexpr int kNcn8MaxGroups = 256;  // resident workgroups of the workspace form: one region each

// the count rows: LDS, or a region of global memory that only this workgroup touches -- its atomics run in L2, so the reads go there too
// (agent-scope loads pass the CU's L1, which may hold the row as an earlier pair left it)
template <bool kLds>
struct Rows;
template <>
struct Rows<true> {
  static __device__ __forceinline__ int ld(const int32_t* p) { return *p; }
  static __device__ __forceinline__ void st(int32_t* p, int v) { *p = v; }
  static __device__ __forceinline__ void add(int32_t* p, int v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  static __device__ __forceinline__ void sync() { __syncthreads(); }
};
template <>
struct Rows<false> {
  static __device__ __forceinline__ int ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ void st(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ void add(int32_t* p, int v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ void sync() {
    __threadfence();
    __syncthreads();
  }
};

// W[r, n] with decay_weight's float32 argument (ncn_rows.h) and the exponential taken in float64: the weighted blocks multiply it onto
// integer counts in the hundreds and sum terms that cancel, where the rounding of a float32 weight shows in cn_emb
__device__ __forceinline__ double decay_weight_f64(const int64_t* __restrict__ last_update, long long et, long long n) {
  const float gap = (float)(et - (long long)last_update[n]);
  return exp(-(double)(gap / 10000.f));
}

// One target's side of the scatter: every wave takes distinct neighbours m of the target (the first entry of a run of equal ids; a = the
// run's length), writes R[m] = a and walks row m, its lanes an entry each: S[n] += a, and sp[n] += a b where m is a neighbour of the other
// target too (b entries in ITS row; `other` empty: no sp).  kClear: store zeros at the same places instead.
template <bool kLds, bool kClear>
__device__ __forceinline__ void ncn8_walk(const int32_t* __restrict__ indptr, const int32_t* __restrict__ cols, int lo, int hi, int olo, int ohi,
                                          int32_t* R, int32_t* S, int32_t* sp) {
  using Rw = Rows<kLds>;
  const int lane = lane_id(), wave = threadIdx.x / kWave;
  for (int p = lo + wave; p < hi; p += kNcn8Waves) {  // (p is the wave's: no divergence)
    const int m = cols[p];
    if (p > lo && cols[p - 1] == m) continue;
    const int a = lower_bound_i32(cols, p, hi, (long long)m + 1) - p;
    const int b = olo < ohi ? count_in(cols, olo, ohi, m) : 0;
    if (lane == 0) Rw::st(R + m, kClear ? 0 : a);
    const int mlo = indptr[m], mhi = indptr[m + 1];
    for (int q = mlo + lane; q < mhi; q += kWave) {
      const int n = cols[q];
      if (kClear) {
        Rw::st(S + n, 0);
        if (b) Rw::st(sp + n, 0);
      } else {
        Rw::add(S + n, a);
        if (b) Rw::add(sp + n, a * b);
      }
    }
  }
}

// sum over the entries p of the row [lo, hi) of S[cols[p]] = sum over m of A[t, m] (A A)[t, m] = K3[t, t]; this thread's share
template <bool kLds>
__device__ __forceinline__ long long ncn8_k3_part(const int32_t* __restrict__ cols, int lo, int hi, const int32_t* S) {
  long long s = 0;
  for (int p = lo + (int)threadIdx.x; p < hi; p += kNcn8Threads) s += Rows<kLds>::ld(S + cols[p]);
  return s;
}

static long long ncn8_groups(long long B) { return B < 1 ? 1 : (B > kNcn8MaxGroups ? kNcn8MaxGroups : B); }
static size_t ncn8_region_ints(long long N) { return ((size_t)kNcn8Rows * (size_t)N + 63) & ~(size_t)63; }

// > 64 KB of LDS per workgroup is a per-device opt-in of the kernel function: `done` is that kernel's own table of kNcn8MaxDevices flags
constexpr int kNcn8MaxDevices = 64;
static bool ncn8_lds_optin(const void* kernel, std::atomic<bool>* done, const char* who) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kNcn8MaxDevices) dev = -1;
  if (dev >= 0 && done[dev].load(std::memory_order_acquire)) return true;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kNcn8Rows * kNcn8LdsMaxN * (int)sizeof(int32_t));
  if (e != hipSuccess) {
    set_error("%s: cannot reserve LDS: %s", who, hipGetErrorString(e));
    return false;
  }
  if (dev >= 0) done[dev].store(true, std::memory_order_release);
  return true;
}

}  // namespace tgmx
