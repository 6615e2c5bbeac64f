// What the NCNPredictor forward (ncn.hip) and its backward (ncn_bwd.hip) both read of the sorted-row adjacency, and the time-decay weight:
// one definition, so the backward's W[r, n] and A[a, b] are the forward's, bit for bit.
#pragma once
#include "common.h"

namespace tgmx {

__device__ __forceinline__ int lower_bound_i32(const int32_t* __restrict__ c, int lo, int hi, long long v) {
  while (lo < hi) {
    const int mid = (int)(((long long)lo + hi) >> 1);
    if ((long long)c[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// how often id v occurs in the sorted run c[lo, hi)
__device__ __forceinline__ int count_in(const int32_t* __restrict__ c, int lo, int hi, long long v) {
  const int a = lower_bound_i32(c, lo, hi, v);
  if (a == hi || c[a] != v) return 0;
  return lower_bound_i32(c, a, hi, v + 1) - a;
}
// exp(-(float32(edge_time - last_update) / 10000)): the int64 gap rounded to float32 as torch does, a correctly rounded division, an accurate expf
__device__ __forceinline__ float decay_weight(const int64_t* __restrict__ last_update, long long et, long long n) {
  const float gap = (float)(et - (long long)last_update[n]);
  return expf(-(gap / 10000.f));
}

// last [2 N] int32: the last position at which every id occurs as a source (last[id]) and as a destination (last[N + id]), -1 where it does
// not; a pair with a target outside [0, N) marks nothing (ncn.hip; the k = 2 / 4 and the k = 8 pair kernels read the same marks)
int ncn_last_marks(const void* tar, int tar_is64, long long tar_stride, long long B, long long N, int32_t* last, hipStream_t st);

}  // namespace tgmx
