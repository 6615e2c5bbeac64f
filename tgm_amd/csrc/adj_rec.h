// The adjacency record of the static index and the rings, the wave search for a node's visible prefix, and what the two
// uniform-sampler kernels share (csrc/recency.hip: k <= 64, csrc/uniform_wide.hip: 64 < k <= 2048).
#pragma once

#include "common.h"

namespace tgmx {

struct __align__(16) Rec {
  int nbr;
  int eid;
  long long ts;
};
static_assert(sizeof(Rec) == sizeof(tgmx_adj_t), "record layout");

// Number of records in [a, z) whose eid < bound, given that those records form
// a prefix (true for batch-boundary bounds).  64 probes/round.
__device__ __forceinline__ long long wave_prefix_count(const Rec* recs, long long a, long long z,
                                                       long long bound, int lane) {
  long long lo = a, hi = z;
  while (hi - lo > kWave) {
    const long long len = hi - lo;
    const long long stride = (len + kWave - 1) / kWave;
    long long idx = lo + (long long)(lane + 1) * stride - 1;
    if (idx > hi - 1) idx = hi - 1;
    const bool less = (long long)recs[idx].eid < bound;
    const int c = __popcll(__ballot(less));
    long long nlo = lo, nhi = hi;
    if (c > 0) {
      long long p = lo + (long long)c * stride - 1;
      if (p > hi - 1) p = hi - 1;
      nlo = p + 1;
    }
    if (c < kWave) {
      long long p = lo + (long long)(c + 1) * stride - 1;
      if (p > hi - 1) p = hi - 1;
      nhi = p;  // recs[p] is >= bound: the answer is <= p
    }
    lo = nlo;
    hi = nhi < nlo ? nlo : nhi;
  }
  const long long idx = lo + lane;
  const bool less = idx < hi && (long long)recs[idx].eid < bound;
  return lo + __popcll(__ballot(less)) - a;
}

struct UniformArgs {
  const int64_t* indptr;
  const Rec* recs;
  const float* edge_x;
  const int32_t* seeds;
  int32_t* out_nid;
  int64_t* out_ts;
  float* out_x;
  int32_t* status;
  long long S, ev_hi;
  unsigned long long rng_seed, rng_stream;
  int D, k, N, allow_pad;
};

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

}  // namespace tgmx
