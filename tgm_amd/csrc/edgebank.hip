// EdgeBankPredictor (the reference's tgm/nn/modules/edgebank.py), for gfx950: the edge memory as a device hash table, the batch update, the
// batched queries (flat, and one source against its destination and its negatives) and the rehash into a larger table.
//
// Table (pairtable.h): open addressing, linear probing, capacity a power of two.  A slot is 16 bytes {uint64 key = src << 32 | dst, int64 ts}, so a probe is
// one 16-byte load; the empty key is all ones (ids lie in [0, 2^31), so no pair packs to it).  A key is written once, by a 64-bit
// compare-and-swap, and never changes or leaves until a rehash: a probe that meets an empty slot has seen every slot the key could be in.
//
// Update: the reference's loop keeps, per pair, the timestamp of the LAST arrival that passed the window test.  Three phases, separated by
// a barrier (one workgroup, up to 1024 events) or a launch boundary (more):
//   1  max(ts) -> the new window end (the window start every later test uses follows from it);
//   2  every in-window event finds or claims its slot and does atomicMax(stamp[slot], g), g = its global arrival number (> 0, growing
//      over calls, so nothing is reset per batch);
//   3  the event whose g is the stamp writes its ts.
// stamp[] is a separate array: only the update touches it, and a query's probe stays one 16-byte load.  Exactly one event per touched slot
// writes, what it writes does not depend on scheduling, and no float takes part in an atomic: two runs give the same contents (slot
// positions may differ with the order in which colliding keys claim).
//
// Every probe loop is a for over at most `capacity` probes; one that runs out sets kOverflow in the status word and gives up.
#include "pairtable.h"

namespace tgmx {

constexpr int kEbBadId = 1, kEbOverflow = 2;  // status bits
constexpr int kEbBlockMax = 1024;             // events the one-workgroup update takes

struct alignas(16) EbState {  // tgmx_edgebank_state_bytes()
  long long end;              // window_end
  long long size_i;           // window size, unlimited mode (int64 arithmetic)
  float size_f;               // window size, fixed mode (float32 arithmetic, as the reference's 0-dim tensors)
  int pad_[3];
};
static_assert(sizeof(EbState) == 32, "edgebank layouts");

__device__ __forceinline__ unsigned long long eb_key(long long s, long long d) { return ((unsigned long long)s << 32) | (unsigned long long)d; }

// the insertion test `ts >= window_start`: float32 on both sides in fixed mode (the reference compares a Python int with a 0-dim float32
// tensor, which rounds the int), int64 otherwise
__device__ __forceinline__ bool eb_in_window(long long ts, long long end, const EbState& s, int fixed) {
  return fixed ? (float)ts >= (float)end - s.size_f : ts >= end - s.size_i;
}
// the query's test: the stored int64 against the float32 start taken exactly (Python compares an int with a float exactly; |ts| < 2^53)
__device__ __forceinline__ bool eb_hit(long long ts, long long end, const EbState& s, int fixed) {
  return !fixed || (double)ts >= (double)((float)end - s.size_f);
}

struct EbUpdateArgs {
  EbSlot* table;
  long long* stamp;
  long long cap;
  EbState* state;
  int fixed;
  long long arrivals;
  int* status;
  const void *src, *dst, *ts;
  int src64, dst64, ts64;
  long long n;
};

__device__ __forceinline__ bool eb_event(const EbUpdateArgs& a, long long e, unsigned long long* key, long long* t) {
  const long long s = ld_idx(a.src, a.src64, e), d = ld_idx(a.dst, a.dst64, e);
  *t = ld_idx(a.ts, a.ts64, e);
  *key = eb_key(s, d);
  return eb_id_ok(s, d);
}
// phase 2 for one event: claim, stamp.  Returns the slot (-1: nothing to write)
__device__ __forceinline__ long long eb_stamp(const EbUpdateArgs& a, unsigned long long key, long long g) {
  const long long slot = eb_claim(a.table, a.cap, key);
  if (slot < 0) {
    atomicOr(a.status, kEbOverflow);
    return -1;
  }
  atomicMax(&a.stamp[slot], g);
  return slot;
}
// phase 3: the stamp is read past the L1 (the atomics ran in L2; a line this CU cached before them would be stale)
__device__ __forceinline__ void eb_write(const EbUpdateArgs& a, long long slot, long long g, long long t) {
  if (slot >= 0 && __hip_atomic_load(&a.stamp[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == g) a.table[slot].val = t;
}

// n <= kEbBlockMax events, one workgroup, one event per thread
__global__ __launch_bounds__(kEbBlockMax) void eb_update_block_kernel(EbUpdateArgs a) {
  __shared__ long long s_max[kEbBlockMax / kWave];
  __shared__ long long s_end;
  const int tid = threadIdx.x;
  unsigned long long key = 0;
  long long t = 0;
  const bool live = tid < a.n && eb_event(a, tid, &key, &t);
  if (tid < a.n && !live) atomicOr(a.status, kEbBadId);
  long long m = live ? t : INT64_MIN;
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const long long o = __shfl_xor(m, off);
    m = o > m ? o : m;
  }
  if (lane_id() == 0) s_max[tid / kWave] = m;
  __syncthreads();
  if (tid == 0) {
    long long end = a.state->end;
    for (int w = 0; w < (int)(blockDim.x / kWave); ++w) end = s_max[w] > end ? s_max[w] : end;
    a.state->end = end;
    s_end = end;
  }
  __syncthreads();
  const EbState st = *a.state;  // the sizes (end: from LDS, the store above is this workgroup's own)
  const long long g = a.arrivals + tid + 1;
  long long slot = -1;
  if (live && eb_in_window(t, s_end, st, a.fixed)) slot = eb_stamp(a, key, g);
  __syncthreads();
  eb_write(a, slot, g, t);
}

// the bulk shape: the same phases as three launches
__global__ __launch_bounds__(kEbThreads) void eb_update_max_kernel(EbUpdateArgs a) {
  __shared__ long long s_max[kEbThreads / kWave];
  const long long step = (long long)gridDim.x * blockDim.x;
  long long m = INT64_MIN;
  bool bad = false;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < a.n; e += step) {
    unsigned long long key;
    long long t;
    if (eb_event(a, e, &key, &t)) m = t > m ? t : m;
    else bad = true;
  }
  if (bad) atomicOr(a.status, kEbBadId);
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const long long o = __shfl_xor(m, off);
    m = o > m ? o : m;
  }
  if (lane_id() == 0) s_max[threadIdx.x / kWave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kEbThreads / kWave; ++w) m = s_max[w] > m ? s_max[w] : m;
    if (m != INT64_MIN) atomicMax(&a.state->end, m);
  }
}
template <bool WRITE>
__global__ __launch_bounds__(kEbThreads) void eb_update_bulk_kernel(EbUpdateArgs a) {
  const EbState st = *a.state;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < a.n; e += step) {
    unsigned long long key;
    long long t;
    if (!eb_event(a, e, &key, &t) || !eb_in_window(t, st.end, st, a.fixed)) continue;
    const long long g = a.arrivals + e + 1;
    if (!WRITE) {
      eb_stamp(a, key, g);
    } else {
      long long unused;
      eb_write(a, eb_find(a.table, a.cap, key, &unused), g, t);  // (absent only after an overflow)
    }
  }
}

struct EbQueryArgs {
  const EbSlot* table;
  long long cap;
  const EbState* state;
  int fixed;
  double pos_prob;
  int* status;
  const void *src, *dst, *neg;
  int src64, dst64, neg64;
  const int64_t* neg_off;  // [B + 1] for ragged rows, NULL: M per row
  long long M, B, total;
  void* out;
  int out_dtype;
};

__global__ __launch_bounds__(kEbThreads) void eb_query_kernel(EbQueryArgs a) {
  const EbState st = *a.state;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.total; i += step) {
    long long b = i, c = 0;  // flat: query i is (src[i], dst[i])
    long long nbase = 0;
    if (a.neg) {  // one against many: row b holds (src[b], dst[b]) then (src[b], neg[b][m])
      if (a.neg_off) {
        long long lo = 0, hi = a.B;  // the last row whose first output index neg_off[b] + b is <= i
        while (hi - lo > 1) {
          const long long mid = (lo + hi) >> 1;
          if ((long long)a.neg_off[mid] + mid <= i) lo = mid;
          else hi = mid;
        }
        b = lo;
        nbase = (long long)a.neg_off[b];
        c = i - nbase - b;
      } else {
        b = i / (a.M + 1);
        c = i - b * (a.M + 1);
        nbase = b * a.M;
      }
    }
    const long long s = ld_idx(a.src, a.src64, b);
    const long long d = c == 0 ? ld_idx(a.dst, a.dst64, b) : ld_idx(a.neg, a.neg64, nbase + c - 1);
    bool hit = false;
    if (eb_id_ok(s, d)) {
      long long ts;
      hit = eb_find(a.table, a.cap, eb_key(s, d), &ts) >= 0 && eb_hit(ts, st.end, st, a.fixed);
    } else {
      atomicOr(a.status, kEbBadId);
    }
    const double v = hit ? a.pos_prob : 0.0;
    switch (a.out_dtype) {
      case 0: reinterpret_cast<int32_t*>(a.out)[i] = (int32_t)v; break;
      case 1: reinterpret_cast<int64_t*>(a.out)[i] = (int64_t)v; break;
      case 2: reinterpret_cast<float*>(a.out)[i] = (float)v; break;
      default: reinterpret_cast<double*>(a.out)[i] = v; break;
    }
  }
}

struct EbRehashArgs {
  const EbSlot* from;
  long long from_cap;
  EbSlot* to;
  long long to_cap;
  const EbState* state;
  int fixed;
  int* status;
  unsigned long long* kept;
};

// fixed mode drops what has left the window (the reference's _clean_up: the insertion test, float32 on both sides)
__global__ __launch_bounds__(kEbThreads) void eb_rehash_kernel(EbRehashArgs a) {
  const EbState st = *a.state;
  eb_move_slots(a.from, a.from_cap, a.to, a.to_cap, a.status, kEbOverflow, a.kept, [&](long long ts) { return eb_in_window(ts, st.end, st, a.fixed); });
}

static bool eb_valid(const tgmx_edgebank_t* eb) {
  return eb && eb->table && eb->stamp && eb->state && eb->status && eb->capacity >= 2 && eb->capacity < (1ll << 40) &&
         (eb->capacity & (eb->capacity - 1)) == 0;
}

}  // namespace tgmx

using namespace tgmx;

extern "C" size_t tgmx_edgebank_state_bytes(void) { return sizeof(EbState); }

extern "C" int tgmx_edgebank_update(const tgmx_edgebank_t* eb, const void* src, int32_t src_is64, const void* dst, int32_t dst_is64, const void* ts,
                                    int32_t ts_is64, int64_t n, tgmx_stream_t stream) {
  TGMX_REQUIRE(eb_valid(eb), "edgebank_update: bad table block (capacity must be a power of two >= 2)");
  TGMX_REQUIRE(n >= 0 && eb->arrivals >= 0, "edgebank_update: bad sizes n=%lld arrivals=%lld", (long long)n, (long long)eb->arrivals);
  if (n == 0) return TGMX_OK;
  TGMX_REQUIRE(src && dst && ts, "edgebank_update: null pointer");
  hipStream_t st = (hipStream_t)stream;
  EbUpdateArgs a{reinterpret_cast<EbSlot*>(eb->table), reinterpret_cast<long long*>(eb->stamp), (long long)eb->capacity,
                 reinterpret_cast<EbState*>(eb->state), eb->fixed != 0, (long long)eb->arrivals, eb->status, src, dst, ts,
                 src_is64 != 0, dst_is64 != 0, ts_is64 != 0, (long long)n};
  if (n <= kEbBlockMax) {
    const unsigned threads = (unsigned)((n + kWave - 1) / kWave * kWave);
    hipLaunchKernelGGL(eb_update_block_kernel, dim3(1), dim3(threads), 0, st, a);
    TGMX_CHECK_LAUNCH("edgebank_update");
    return TGMX_OK;
  }
  hipLaunchKernelGGL(eb_update_max_kernel, dim3(eb_grid(n)), dim3(kEbThreads), 0, st, a);
  TGMX_CHECK_LAUNCH("edgebank_update(max)");
  hipLaunchKernelGGL(eb_update_bulk_kernel<false>, dim3(eb_grid(n)), dim3(kEbThreads), 0, st, a);
  TGMX_CHECK_LAUNCH("edgebank_update(stamp)");
  hipLaunchKernelGGL(eb_update_bulk_kernel<true>, dim3(eb_grid(n)), dim3(kEbThreads), 0, st, a);
  TGMX_CHECK_LAUNCH("edgebank_update(write)");
  return TGMX_OK;
}

extern "C" int tgmx_edgebank_query(const tgmx_edgebank_t* eb, const void* src, int32_t src_is64, const void* dst, int32_t dst_is64, const void* neg,
                                   int32_t neg_is64, const int64_t* neg_off, int64_t M, int64_t B, int64_t total, void* out, int32_t out_dtype,
                                   tgmx_stream_t stream) {
  TGMX_REQUIRE(eb_valid(eb), "edgebank_query: bad table block (capacity must be a power of two >= 2)");
  TGMX_REQUIRE(B >= 0 && total >= 0 && M >= 0 && out_dtype >= 0 && out_dtype <= 3, "edgebank_query: bad sizes B=%lld total=%lld M=%lld out_dtype=%d",
               (long long)B, (long long)total, (long long)M, out_dtype);
  TGMX_REQUIRE(neg || neg_off || total == B, "edgebank_query: the flat form answers one query per pair (total=%lld, B=%lld)", (long long)total, (long long)B);
  TGMX_REQUIRE(!neg || neg_off || total == B * (M + 1), "edgebank_query: [B, M] negatives give B (M + 1) answers (total=%lld)", (long long)total);
  TGMX_REQUIRE(!neg_off || neg, "edgebank_query: row offsets without negatives");
  if (total == 0) return TGMX_OK;
  TGMX_REQUIRE(src && dst && out && B > 0, "edgebank_query: null pointer");
  EbQueryArgs a{reinterpret_cast<const EbSlot*>(eb->table), (long long)eb->capacity, reinterpret_cast<const EbState*>(eb->state), eb->fixed != 0,
                eb->pos_prob, eb->status, src, dst, neg, src_is64 != 0, dst_is64 != 0, neg_is64 != 0, neg_off, (long long)M, (long long)B,
                (long long)total, out, out_dtype};
  hipLaunchKernelGGL(eb_query_kernel, dim3(eb_grid(total)), dim3(kEbThreads), 0, (hipStream_t)stream, a);
  TGMX_CHECK_LAUNCH("edgebank_query");
  return TGMX_OK;
}

extern "C" int tgmx_edgebank_rehash(const tgmx_edgebank_t* from, const tgmx_edgebank_t* to, int64_t* kept, tgmx_stream_t stream) {
  TGMX_REQUIRE(eb_valid(from) && eb_valid(to) && kept, "edgebank_rehash: bad table block");
  TGMX_REQUIRE(to->capacity >= 2 * from->capacity && to->table != from->table, "edgebank_rehash: the new table must be at least twice the old (%lld -> %lld)",
               (long long)from->capacity, (long long)to->capacity);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(kept, 0, sizeof(int64_t), st) != hipSuccess) {
    set_error("edgebank_rehash: clearing the count failed");
    return TGMX_E_LAUNCH;
  }
  EbRehashArgs a{reinterpret_cast<const EbSlot*>(from->table), (long long)from->capacity, reinterpret_cast<EbSlot*>(to->table), (long long)to->capacity,
                 reinterpret_cast<const EbState*>(from->state), from->fixed != 0, to->status, reinterpret_cast<unsigned long long*>(kept)};
  hipLaunchKernelGGL(eb_rehash_kernel, dim3(eb_grid(from->capacity)), dim3(kEbThreads), 0, st, a);
  TGMX_CHECK_LAUNCH("edgebank_rehash");
  return TGMX_OK;
}
