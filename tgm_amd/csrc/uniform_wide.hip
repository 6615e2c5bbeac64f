// Uniform temporal neighbor sampling for 64 < k <= 2048 (NeighborSamplerHook; tgmx_uniform_lookup_wide) for gfx950.
//
// The draw is the one uniform_lookup_kernel (csrc/recency.hip, k <= 64) defines: for a node with c > k candidates, step i in
// [0, k) of a Fisher-Yates shuffle of the virtual identity array a over [0, c) picks j_i = i + umul64hi(splitmix64(base + i), c - i),
// output slot i takes a[j_i], then a[j_i] = a[i].  That kernel walks the k steps as one serial chain inside a wave, with the array's
// overrides one per lane; neither stretches past 64.  Here the chain is gone:
//
//   every j_i depends on i alone, so all k are computed at once.  What is left is which earlier write each read sees.  A write
//   to position p can only come from a step i' < p (j >= i), so
//     val(i), the value step i moves out of a[i], is val(q) for q = max{i'' < i : j_i'' = i}, and i when there is none: a forest
//       over [0, k) whose parents have smaller indices;
//     slot i's output is val(q) for q = max{i' < i : j_i' = j_i}, and j_i when there is none.
//   Both q's are neighbours in the order of the pairs (j, i): q of slot i is the pair in front of (j_i, i) when that has the same
//   j, and the parent of position t is the last pair of the run with j = t that is not (t, t) itself.
//
// Work split: ONE workgroup of four waves per seed (grid-stride over the seeds), the whole draw in LDS, 18 bytes per slot:
//   0. wave 0 finds the seed's candidate count c with the 64-ary prefix search and publishes it; c <= k skips to 4 (slot j takes
//      candidate j, the rest are pads)
//   1. k hashes -> (j, i) pairs, padded to kp = the next power of two with j = max
//   2. bitonic sort of the kp pairs by (j, i): j stays 64-bit (c is), i is 16-bit
//   3. parents from neighbouring pairs, then log2(kp) rounds of pointer jumping between two 16-bit arrays: root(i) = val(i)
//   4. every sorted pair resolves its slot's candidate, reads the record and writes id and time; the edge id goes to LDS
//   5. the four waves copy the k feature rows, a coalesced row per wave trip (pad slots: zeros), in 16-byte pieces when D % 4 == 0
// A wave per short seed (k <= 256) was the alternative for steps 1-4; step 5 moves nearly all of the bytes and wants all four waves
// on one seed's rows, so the split is the same at every k.  No atomics but the status word's.
#include <limits.h>

#include "adj_rec.h"
#include "common.h"

namespace tgmx {

constexpr int kWideThreads = 256;
constexpr int kWideMaxK = 2048;
constexpr int kWideSlotBytes = 8 + 4 + 2 + 2 + 2;  // s_j, s_eid, s_i, two parent arrays

__device__ __forceinline__ void set_zero(float& v) { v = 0.f; }
__device__ __forceinline__ void set_zero(float4& v) { v = make_float4(0.f, 0.f, 0.f, 0.f); }

// Step 5: the seed's k feature rows (row_vecs elements of V each; rows of edge_x addressed by the edge ids in LDS, -1: a zero row).
// A wave trip copies a row, coalesced; wave w takes rows w and w + 4 of every eight together, two pieces of each: four loads in
// flight per lane ahead of their stores.
template <typename V>
__device__ __forceinline__ void copy_rows(const float* edge_x, float* out, const int* s_eid, int k, int row_vecs, int wave, int lane) {
  constexpr int kWaves = kWideThreads / kWave;
  const V* __restrict__ xs = reinterpret_cast<const V*>(edge_x);
  V* __restrict__ os = reinterpret_cast<V*>(out);
  for (int row0 = wave; row0 < k; row0 += 2 * kWaves) {
    const int row1 = row0 + kWaves;
    const int e0 = s_eid[row0], e1 = row1 < k ? s_eid[row1] : -1;
    for (int c0 = lane; c0 < row_vecs; c0 += 2 * kWave) {
      V v0[2], v1[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int col = c0 + u * kWave;
        set_zero(v0[u]);
        set_zero(v1[u]);
        if (col < row_vecs) {
          if (e0 >= 0) v0[u] = xs[(long long)e0 * row_vecs + col];
          if (e1 >= 0) v1[u] = xs[(long long)e1 * row_vecs + col];
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int col = c0 + u * kWave;
        if (col < row_vecs) {
          os[(long long)row0 * row_vecs + col] = v0[u];
          if (row1 < k) os[(long long)row1 * row_vecs + col] = v1[u];
        }
      }
    }
  }
}

__global__ __launch_bounds__(kWideThreads) void uniform_lookup_wide_kernel(const UniformArgs a, const int kp, const int vec4) {
  extern __shared__ __align__(16) unsigned char wide_lds[];
  long long* s_j = reinterpret_cast<long long*>(wide_lds);         // [kp] the pairs' j
  int* s_eid = reinterpret_cast<int*>(s_j + kp);                    // [kp] edge id behind slot i (-1: pad)
  unsigned short* s_i = reinterpret_cast<unsigned short*>(s_eid + kp);  // [kp] the pairs' i
  unsigned short* s_par = s_i + kp;                                 // [2][kp] forest pointers, ping-pong
  __shared__ long long s_head[2];                                   // the seed's row start and candidate count
  const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  const int k = a.k;
  const int rounds = 31 - __clz(kp);  // 2^rounds = kp >= k > the deepest chain
  for (long long s = blockIdx.x; s < a.S; s += gridDim.x) {
    const int n = a.seeds[s];
    // ---- 0. candidate count, once per seed ----
    if (wave == 0) {
      const bool live = n >= 0 && n < a.N;
      if (lane == 0 && (n >= a.N || n < -1 || (n == -1 && !a.allow_pad))) atomicOr(a.status, TGMX_ST_SEED_RANGE);
      long long ra = 0, c = 0;
      if (live) {
        ra = a.indptr[n];
        c = wave_prefix_count(a.recs, ra, a.indptr[n + 1], a.ev_hi, lane);
      }
      if (lane == 0) {
        s_head[0] = ra;
        s_head[1] = c;
      }
    }
    __syncthreads();
    const long long ra = s_head[0], c = s_head[1];
    int32_t* __restrict__ o_nid = a.out_nid + s * k;
    int64_t* __restrict__ o_ts = a.out_ts + s * k;
    if (c <= k) {
      for (int i = tid; i < k; i += kWideThreads) {
        int nid = -1, eid = -1;
        long long ts = 0;
        if (i < c) {
          const Rec r = a.recs[ra + i];
          nid = r.nbr;
          ts = r.ts;
          eid = r.eid;
        }
        o_nid[i] = nid;
        o_ts[i] = ts;
        s_eid[i] = eid;
      }
    } else {
      // ---- 1. the k picks ----
      const unsigned long long base = splitmix64(a.rng_seed ^ splitmix64(a.rng_stream ^ ((unsigned long long)(unsigned)n << 32)));
      for (int i = tid; i < kp; i += kWideThreads) {
        long long j = LLONG_MAX;  // pads sort behind every pick (j < c)
        if (i < k) {
          const unsigned long long r = splitmix64(base + (unsigned long long)i);
          j = i + (long long)__umul64hi(r, (unsigned long long)(c - i));  // uniform in [i, c)
          s_par[i] = (unsigned short)i;
        }
        s_j[i] = j;
        s_i[i] = (unsigned short)i;
      }
      __syncthreads();
      // ---- 2. sort the pairs by (j, i) ----
      for (int size = 2; size <= kp; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
          for (int t = tid; t < (kp >> 1); t += kWideThreads) {
            const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), hi = lo + stride;
            const long long jl = s_j[lo], jh = s_j[hi];
            const unsigned short il = s_i[lo], ih = s_i[hi];
            const bool after = jl > jh || (jl == jh && il > ih);
            if (after == ((lo & size) == 0)) {
              s_j[lo] = jh;
              s_j[hi] = jl;
              s_i[lo] = ih;
              s_i[hi] = il;
            }
          }
          __syncthreads();
        }
      }
      // ---- 3. the forest: the picks sit in the first k sorted positions.  A pair (t, i) with i < t < k is a write into a position
      // that step t reads as a[t]; the last such pair of its run (the run's only possible later pair is (t, t)) is t's parent ----
      for (int p = tid; p < k; p += kWideThreads) {
        const long long j = s_j[p];
        const int i = s_i[p];
        if (j < k && i < j) {
          if (p + 1 == kp || s_j[p + 1] != j || (long long)s_i[p + 1] == j) s_par[(int)j] = (unsigned short)i;
        }
      }
      __syncthreads();
      unsigned short* cur = s_par;
      unsigned short* nxt = s_par + kp;
      for (int r = 0; r < rounds; ++r) {
        for (int i = tid; i < k; i += kWideThreads) nxt[i] = cur[cur[i]];
        __syncthreads();
        unsigned short* t = cur;
        cur = nxt;
        nxt = t;
      }
      // ---- 4. slot i of pair (j, i) takes val(pair in front) when that has the same j, else candidate j ----
      for (int p = tid; p < k; p += kWideThreads) {
        const long long j = s_j[p];
        const int i = s_i[p];
        long long pick = j;
        if (p > 0 && s_j[p - 1] == j) pick = cur[s_i[p - 1]];
        const Rec r = a.recs[ra + pick];
        o_nid[i] = r.nbr;
        o_ts[i] = r.ts;
        s_eid[i] = r.eid;
      }
    }
    __syncthreads();
    // ---- 5. features ----
    if (a.D > 0) {
      float* o = a.out_x + s * (long long)k * a.D;
      if (vec4) copy_rows<float4>(a.edge_x, o, s_eid, k, a.D >> 2, wave, lane);
      else copy_rows<float>(a.edge_x, o, s_eid, k, a.D, wave, lane);
    }
    __syncthreads();  // the next seed reuses s_head and s_eid
  }
}

}  // namespace tgmx

using namespace tgmx;

extern "C" int tgmx_uniform_lookup_wide(const int64_t* indptr, const tgmx_adj_t* adj, const float* edge_x, int32_t D,
                                        const int32_t* seeds, int64_t S, int32_t k, int64_t ev_hi, int32_t num_nodes,
                                        int32_t allow_pad, uint64_t rng_seed, uint64_t rng_stream, int32_t* out_nid,
                                        int64_t* out_ts, float* out_x, int32_t* status, tgmx_stream_t stream) {
  TGMX_REQUIRE(k > kWave && k <= kWideMaxK, "uniform_lookup_wide: k=%d outside (64, %d] (k <= 64: tgmx_uniform_lookup_csr)", k, kWideMaxK);
  TGMX_REQUIRE(S >= 0 && D >= 0 && num_nodes > 0 && ev_hi >= 0, "uniform_lookup_wide: bad sizes S=%lld D=%d N=%d", (long long)S, D, num_nodes);
  if (S == 0) return TGMX_OK;
  TGMX_REQUIRE(indptr && adj && seeds && out_nid && out_ts && status, "uniform_lookup_wide: null pointer");
  TGMX_REQUIRE(D == 0 || (edge_x && out_x), "uniform_lookup_wide: D=%d but edge_x/out_x is null", D);
  TGMX_REQUIRE(((uintptr_t)adj & 15) == 0, "uniform_lookup_wide: adj must be 16-byte aligned");
  UniformArgs a{indptr, reinterpret_cast<const Rec*>(adj), edge_x, seeds, out_nid, out_ts, out_x, status, S, ev_hi,
                (unsigned long long)rng_seed, (unsigned long long)rng_stream, D, k, num_nodes, allow_pad};
  int kp = 2 * kWave;
  while (kp < k) kp <<= 1;
  const long long blocks = S < (1 << 20) ? S : (1 << 20);
  // rows as 16-byte pieces where they are (every row of edge_x and of out_x then starts on a 16-byte boundary)
  const int vec4 = D > 0 && D % 4 == 0 && (((uintptr_t)edge_x | (uintptr_t)out_x) & 15) == 0;
  hipLaunchKernelGGL(uniform_lookup_wide_kernel, dim3((unsigned)blocks), dim3(kWideThreads), (size_t)kp * kWideSlotBytes, (hipStream_t)stream, a, kp,
                     vec4);
  TGMX_CHECK_LAUNCH("uniform_lookup_wide");
  return TGMX_OK;
}
