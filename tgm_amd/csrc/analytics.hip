// BatchAnalyticsHook, EdgeEventsSeenNodesTrackHook and NodeAnalyticsHook (the reference's tgm/hooks/analytics/, tgm/hooks/node_tracks.py) for
// gfx950.  The reference answers each with torch.unique / nonzero / .item() round trips and Python loops over the events; all three are small
// set-membership problems:
//
//   tgmx_batch_analytics      distinct counts within a batch: five batch-local hash sets, one insert launch
//   tgmx_seen_nodes_step      a byte mask that grows over the stream + an ordered compaction of the labelled nodes it holds
//   tgmx_node_analytics_step  four pair tables (pairtable.h) that grow over the stream: who claims a slot first knows the key is new
//
// The distinct counter.  A set is an array of int32 slots, a power of two >= 2 x its keys, that hold the INDEX of the key that claimed them
// (-1: empty; claimed by a 32-bit compare-and-swap).  A key that meets a taken slot reads the claimer's key from the INPUT arrays, which no
// launch writes: equal = a duplicate, else probe on (at most `capacity` probes).  So a key may be of any width -- an id, a time, a
// (src, dst, time) triple -- without a slot wider than 4 bytes, and nothing is ever read half-written.  Exactly one occurrence of every
// distinct key claims a slot, whichever it is: the count (one integer add per wave after a ballot) does not depend on scheduling.
//
// Everything the launches of one call hand to each other crosses a launch boundary; inside a launch threads meet only in atomics.
#include "pairtable.h"

namespace tgmx {

constexpr int kAnThreads = 256;
constexpr int kAnSets = 5;          // all ids, edge endpoint ids, times, (src, dst, time), (nid, time)
constexpr int kSnThreads = 1024;    // the compaction's one workgroup: 16 waves

__device__ __forceinline__ bool an_id_ok(long long v, long long N) { return v >= 0 && v < N; }

// ---- tgmx_batch_analytics -------------------------------------------------------------------------------------------------------------

struct AnKey {
  long long a, b, c;
};
__device__ __forceinline__ bool operator==(const AnKey& x, const AnKey& y) { return x.a == y.a && x.b == y.b && x.c == y.c; }

struct BaArgs {
  tgmx_an_batch_t b;
  int time_as_f32;
  long long n[kAnSets];      // keys per set
  long long first[kAnSets];  // first item of the set in the launch's item space
  long long total;
  int* slots[kAnSets];
  unsigned mask[kAnSets];    // capacity - 1
  unsigned long long* counts;  // [8]: distinct keys per set
  long long slots_total;
  int64_t* out;
};

__device__ __forceinline__ long long ba_time(const BaArgs& a, long long i) {  // element i of edge_time u node_time
  const long long t = i < a.b.Et ? ld_idx(a.b.edge_time, a.b.edge_time_is64, i) : ld_idx(a.b.node_time, a.b.node_time_is64, i - a.b.Et);
  return a.time_as_f32 ? (long long)__float_as_int((float)t) : t;  // integers never round to -0.0 or NaN: equal floats have equal bits
}
__device__ __forceinline__ long long ba_id(const BaArgs& a, long long i) {  // element i of src u dst u nids
  if (i < a.b.E) return ld_idx(a.b.src, a.b.src_is64, i);
  if (i < 2 * a.b.E) return ld_idx(a.b.dst, a.b.dst_is64, i - a.b.E);
  return ld_idx(a.b.nids, a.b.nids_is64, i - 2 * a.b.E);
}
__device__ __forceinline__ AnKey ba_key(const BaArgs& a, int set, long long i) {
  switch (set) {
    case 0:
    case 1: return AnKey{ba_id(a, i), 0, 0};
    case 2: return AnKey{ba_time(a, i), 0, 0};
    case 3: return AnKey{ld_idx(a.b.src, a.b.src_is64, i), ld_idx(a.b.dst, a.b.dst_is64, i), ld_idx(a.b.edge_time, a.b.edge_time_is64, i)};
    default: return AnKey{ld_idx(a.b.nids, a.b.nids_is64, i), ld_idx(a.b.node_time, a.b.node_time_is64, i), 0};
  }
}
__device__ __forceinline__ unsigned long long ba_hash(const AnKey& k, int set) {
  unsigned long long h = eb_hash((unsigned long long)k.a);
  if (set >= 3) h = eb_hash(h ^ (unsigned long long)k.b ^ 0x9E3779B97F4A7C15ull);
  if (set == 3) h = eb_hash(h ^ (unsigned long long)k.c ^ 0xD1B54A32D192ED03ull);
  return h;
}

// true when key i of `set` is the first of its value to arrive (it claimed a slot)
__device__ __forceinline__ bool ba_insert(const BaArgs& a, int set, long long i) {
  const AnKey key = ba_key(a, set, i);
  int* slots = a.slots[set];
  const unsigned mask = a.mask[set];
  unsigned s = (unsigned)ba_hash(key, set) & mask;
  for (unsigned p = 0; p <= mask; ++p) {
    int cur = __hip_atomic_load(&slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == -1) {
      cur = atomicCAS(&slots[s], -1, (int)i);
      if (cur == -1) return true;
    }
    if (cur >= 0 && cur < a.n[set] && ba_key(a, set, cur) == key) return false;
    s = (s + 1) & mask;
  }
  return false;  // not reached: the set has room for twice its keys
}

__global__ __launch_bounds__(kAnThreads) void ba_reset_kernel(BaArgs a) {
  const long long step = (long long)gridDim.x * blockDim.x;
  int* slots = a.slots[0];  // the five sets are one contiguous array
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.slots_total; i += step) slots[i] = -1;
  if (blockIdx.x == 0 && threadIdx.x < 8) a.counts[threadIdx.x] = 0;
}

__global__ __launch_bounds__(kAnThreads) void ba_insert_kernel(BaArgs a) {
  const long long step = (long long)gridDim.x * blockDim.x;
  const long long trips = (a.total + step - 1) / step;
  for (long long r = 0; r < trips; ++r) {  // every lane takes every trip (the ballots)
    const long long item = r * step + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int set = -1;
    bool first = false;
    if (item < a.total) {
      set = 0;
#pragma unroll
      for (int k = 1; k < kAnSets; ++k) set += item >= a.first[k];
      first = ba_insert(a, set, item - a.first[set]);
    }
#pragma unroll
    for (int k = 0; k < kAnSets; ++k) {
      const unsigned long long firsts = __ballot(first && set == k);
      if (firsts && lane_id() == 0) atomicAdd(&a.counts[k], (unsigned long long)__popcll(firsts));
    }
  }
}

__global__ void ba_finish_kernel(BaArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long long E = a.b.E, Nn = a.b.Nn;
  const long long u_edge = (long long)a.counts[1];
  a.out[0] = E;
  a.out[1] = Nn;
  a.out[2] = (long long)a.counts[2];
  a.out[3] = (long long)a.counts[0];
  a.out[4] = 0;
  reinterpret_cast<float*>(a.out + 4)[0] = E > 0 ? (float)(2 * E) / (float)u_edge : 0.f;
  a.out[5] = a.n[3] > 0 ? E - (long long)a.counts[3] : 0;
  a.out[6] = a.n[4] > 0 ? Nn - (long long)a.counts[4] : 0;
  a.out[7] = u_edge;
}

static long long an_pow2_slots(long long keys) {
  long long cap = 64;
  while (cap < 2 * keys) cap <<= 1;
  return cap;
}
static void ba_set_sizes(long long E, long long Et, long long Nn, long long Nt, long long n[kAnSets]) {
  n[0] = 2 * E + Nn;
  n[1] = 2 * E;
  n[2] = Et + Nt;
  n[3] = (Et == E) ? E : 0;
  n[4] = (Nt == Nn) ? Nn : 0;
}
static bool ba_sizes_ok(long long E, long long Et, long long Nn, long long Nt) {
  const long long lim = 1ll << 28;
  return E >= 0 && E < lim && Nn >= 0 && Nn < lim && (Et == 0 || Et == E) && (Nt >= 0 && Nt < lim);
}

// ---- tgmx_seen_nodes_step ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kAnThreads) void sn_mark_kernel(uint8_t* mask, long long N, const void* src, int src64, const void* dst, int dst64,
                                                            long long E, unsigned long long* status) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * E; i += step) {
    const long long v = i < E ? ld_idx(src, src64, i) : ld_idx(dst, dst64, i - E);
    if (an_id_ok(v, N)) mask[v] = 1;  // racing stores of one value
    else atomicOr(status, (unsigned long long)TGMX_AN_BAD_ID);
  }
}

// ONE workgroup strides over chunks of kSnThreads positions: within a wave ballot + popcount, a prefix over the workgroup's waves, the base
// carried from chunk to chunk -- the output order is the input order.
__global__ __launch_bounds__(kSnThreads) void sn_compact_kernel(const uint8_t* __restrict__ mask, long long N, const void* __restrict__ nids, int nids64,
                                                              long long Ny, int64_t* __restrict__ out_pos, void* __restrict__ out_ids,
                                                              long long* count, unsigned long long* status) {
  __shared__ int wave_tot[kSnThreads / kWave];
  __shared__ long long carry;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  if (tid == 0) carry = 0;
  __syncthreads();
  bool bad = false;
  for (long long r0 = 0; r0 < Ny; r0 += kSnThreads) {
    const long long i = r0 + tid;
    long long v = 0;
    bool sel = false;
    if (i < Ny) {
      v = ld_idx(nids, nids64, i);
      if (an_id_ok(v, N)) sel = mask[v] != 0;
      else bad = true;
    }
    const unsigned long long b = __ballot(sel);
    if (lane == 0) wave_tot[wave] = __popcll(b);
    __syncthreads();
    long long base = carry;
    for (int w = 0; w < wave; ++w) base += wave_tot[w];
    if (sel) {
      const long long o = base + __popcll(b & ((1ull << lane) - 1ull));
      out_pos[o] = i;
      if (nids64) static_cast<int64_t*>(out_ids)[o] = v;
      else static_cast<int32_t*>(out_ids)[o] = (int32_t)v;
    }
    __syncthreads();  // everybody has read carry and wave_tot
    if (tid == kSnThreads - 1) carry = base + __popcll(b);
    __syncthreads();
  }
  if (tid == 0) *count = carry;
  if (bad) atomicOr(status, (unsigned long long)TGMX_AN_BAD_ID);
}

// ---- tgmx_node_analytics_step -----------------------------------------------------------------------------------------------------------

// scalars: two blocks of 8 int64, call c works in block c & 1 and leaves the other one zero for call c + 1
enum { kNaCur = 0, kNaNewEdges = 1, kNaU = 2, kNaE = 3, kNaNn = 4, kNaNewNodes = 5 };
// counters
enum { kNaTimes = 0, kNaOccEdges = 1, kNaOccNbrs = 2, kNaOccApps = 3, kNaStatus = 4 };

struct NaArgs {
  tgmx_node_analytics_t st;
  tgmx_an_batch_t b;
  long long call;
  int64_t* out;
};

__device__ __forceinline__ unsigned long long* na_u64(int64_t* p) { return reinterpret_cast<unsigned long long*>(p); }
__device__ __forceinline__ void na_flag(const NaArgs& a, int bit) { atomicOr(na_u64(a.st.counters + kNaStatus), (unsigned long long)bit); }
__device__ __forceinline__ void na_count(int64_t* p) { atomicAdd(na_u64(p), 1ull); }

// edge i takes part: both ids in range and its time (if any) not negative; *t: the time, -1 without
__device__ __forceinline__ bool na_edge(const NaArgs& a, long long i, long long* s, long long* d, long long* t) {
  *s = ld_idx(a.b.src, a.b.src_is64, i);
  *d = ld_idx(a.b.dst, a.b.dst_is64, i);
  *t = i < a.b.Et ? ld_idx(a.b.edge_time, a.b.edge_time_is64, i) : -1;
  int bits = 0;
  if (!an_id_ok(*s, a.st.num_nodes) || !an_id_ok(*d, a.st.num_nodes)) bits |= TGMX_AN_BAD_ID;
  if (i < a.b.Et && *t < 0) bits |= TGMX_AN_BAD_TIME;
  if (bits) na_flag(a, bits);
  return bits == 0;
}
__device__ __forceinline__ bool na_node_event(const NaArgs& a, long long j, long long* n, long long* t) {
  *n = ld_idx(a.b.nids, a.b.nids_is64, j);
  *t = j < a.b.Nt ? ld_idx(a.b.node_time, a.b.node_time_is64, j) : -1;
  int bits = 0;
  if (!an_id_ok(*n, a.st.num_nodes)) bits |= TGMX_AN_BAD_ID;
  if (j < a.b.Nt && *t < 0) bits |= TGMX_AN_BAD_TIME;
  if (bits) na_flag(a, bits);
  return bits == 0;
}

// every time of the batch claims its slot; a new one takes the next dense id
__global__ __launch_bounds__(kAnThreads) void na_time_kernel(NaArgs a) {
  const long long step = (long long)gridDim.x * blockDim.x, total = a.b.Et + a.b.Nt;
  int64_t* sc = a.st.scalars + 8 * (a.call & 1);
  EbSlot* times = static_cast<EbSlot*>(a.st.times);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
    long long t, x, y;
    bool ok;
    if (i < a.b.Et) {
      if (i < a.b.E) ok = na_edge(a, i, &x, &y, &t);
      else ok = (t = ld_idx(a.b.edge_time, a.b.edge_time_is64, i)) >= 0;  // a time without an edge (edge_src is None)
    } else {
      const long long j = i - a.b.Et;
      if (j < a.b.Nn) ok = na_node_event(a, j, &x, &t);
      else ok = (t = ld_idx(a.b.node_time, a.b.node_time_is64, j)) >= 0;
    }
    if (!ok) {
      if (t < 0) na_flag(a, TGMX_AN_BAD_TIME);
      continue;
    }
    bool fresh;
    const long long slot = eb_claim_fresh(times, a.st.times_cap, (unsigned long long)t, &fresh);
    if (slot < 0) {
      na_flag(a, TGMX_AN_TABLE_FULL);
      continue;
    }
    if (fresh) {
      const unsigned long long id = atomicAdd(na_u64(a.st.counters + kNaTimes), 1ull);
      if (id >> 32) na_flag(a, TGMX_AN_BAD_TIME);  // more than 2^32 distinct times
      times[slot].val = (long long)id;
    }
    atomicMax(reinterpret_cast<long long*>(sc + kNaCur), t);
  }
}

// (tracked index, time) into the appearances table; the time's dense id was stored a launch ago
__device__ __forceinline__ void na_appear(const NaArgs& a, int idx, long long t) {
  long long tid;
  if (eb_find(static_cast<const EbSlot*>(a.st.times), a.st.times_cap, (unsigned long long)t, &tid) < 0) return;  // its claim found no room
  bool fresh;
  const long long slot = eb_claim_fresh(static_cast<EbSlot*>(a.st.apps), a.st.apps_cap, ((unsigned long long)idx << 32) | (unsigned long long)(tid & 0xFFFFFFFFll), &fresh);
  if (slot < 0) na_flag(a, TGMX_AN_TABLE_FULL);
  else if (fresh) {
    na_count(a.st.appearances + idx);
    na_count(a.st.counters + kNaOccApps);
  }
}

__device__ __forceinline__ void na_endpoint(const NaArgs& a, int64_t* sc, long long x, long long nbr, long long t) {
  if (atomicExch(&a.st.stamp[x], (int)a.call) != (int)a.call) na_count(sc + kNaU);
  const int idx = a.st.slot_of[x];
  if (idx < 0 || idx >= a.st.T) return;
  atomicAdd(&a.st.degree[idx], 1);
  a.st.present[idx] = 1;
  bool fresh;
  const long long slot = eb_claim_fresh(static_cast<EbSlot*>(a.st.nbrs), a.st.nbrs_cap, ((unsigned long long)idx << 32) | (unsigned long long)nbr, &fresh);
  if (slot < 0) na_flag(a, TGMX_AN_TABLE_FULL);
  else if (fresh) {
    atomicAdd(&a.st.new_nbrs[idx], 1);
    na_count(a.st.counters + kNaOccNbrs);
  }
  if (t >= 0) na_appear(a, idx, t);
}

__global__ __launch_bounds__(kAnThreads) void na_event_kernel(NaArgs a) {
  const long long step = (long long)gridDim.x * blockDim.x, total = a.b.E + a.b.Nn;
  int64_t* sc = a.st.scalars + 8 * (a.call & 1);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
    if (i < a.b.E) {
      long long s, d, t;
      if (!na_edge(a, i, &s, &d, &t)) continue;
      na_count(sc + kNaE);
      bool fresh;
      const long long slot = eb_claim_fresh(static_cast<EbSlot*>(a.st.edges), a.st.edges_cap, ((unsigned long long)s << 32) | (unsigned long long)d, &fresh);
      if (slot < 0) na_flag(a, TGMX_AN_TABLE_FULL);
      else if (fresh) {
        na_count(sc + kNaNewEdges);
        na_count(a.st.counters + kNaOccEdges);
      }
      na_endpoint(a, sc, s, d, t);
      na_endpoint(a, sc, d, s, t);
    } else {
      long long n, t;
      if (!na_node_event(a, i - a.b.E, &n, &t)) continue;
      na_count(sc + kNaNn);
      const int idx = a.st.slot_of[n];
      if (idx < 0 || idx >= a.st.T) {
        na_count(sc + kNaNewNodes);
        continue;
      }
      a.st.present[idx] = 1;
      if (t >= 0) na_appear(a, idx, t);
    }
  }
}

__global__ __launch_bounds__(kAnThreads) void na_finalise_kernel(NaArgs a) {
  const long long step = (long long)gridDim.x * blockDim.x, T = a.st.T;
  int64_t* sc = a.st.scalars + 8 * (a.call & 1);
  int64_t* sc_next = a.st.scalars + 8 * ((a.call + 1) & 1);
  const long long cur = sc[kNaCur];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < T + 2; i += step) {
    int64_t row[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i < T) {
      if (a.st.present[i]) {
        if (a.st.first_seen[i] < 0) a.st.first_seen[i] = cur;
        a.st.last_seen[i] = cur;
        row[0] = 2, row[1] = a.st.degree[i], row[2] = a.st.appearances[i], row[3] = a.st.new_nbrs[i], row[4] = cur - a.st.first_seen[i];
      } else if (a.st.last_seen[i] >= 0) {
        row[0] = 1, row[2] = a.st.appearances[i], row[4] = a.st.last_seen[i] - a.st.first_seen[i], row[5] = cur - a.st.last_seen[i];
      }
      a.st.present[i] = 0, a.st.degree[i] = 0, a.st.new_nbrs[i] = 0;
    } else if (i == T) {
      row[0] = a.st.counters[kNaTimes], row[1] = sc[kNaNewEdges], row[2] = sc[kNaU], row[3] = sc[kNaE], row[4] = sc[kNaNn], row[5] = sc[kNaNewNodes];
      row[6] = cur, row[7] = a.st.counters[kNaStatus];
    } else {
      row[0] = a.st.counters[kNaOccEdges], row[1] = a.st.counters[kNaOccNbrs], row[2] = a.st.counters[kNaTimes], row[3] = a.st.counters[kNaOccApps];
      for (int k = 0; k < 8; ++k) sc_next[k] = 0;  // the block call + 1 works in (nobody reads it in this call)
    }
    for (int k = 0; k < 8; ++k) a.out[i * 8 + k] = row[k];
  }
}

// pairtable.h's rehash, keeping every entry.  Its status word is an int: the low half of the counters' little-endian int64, which no other
// launch touches meanwhile.
__global__ __launch_bounds__(kEbThreads) void na_rehash_kernel(const EbSlot* __restrict__ from, long long from_cap, EbSlot* __restrict__ to, long long to_cap,
                                                             int64_t* state) {
  eb_move_slots(from, from_cap, to, to_cap, reinterpret_cast<int*>(state), TGMX_AN_TABLE_FULL, na_u64(state + 1), [](long long) { return true; });
}

static bool an_pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }

}  // namespace tgmx

using namespace tgmx;

extern "C" size_t tgmx_batch_analytics_workspace_bytes(int64_t E, int64_t Et, int64_t Nn, int64_t Nt) {
  if (!ba_sizes_ok(E, Et, Nn, Nt)) return 0;
  long long n[kAnSets], slots = 0;
  ba_set_sizes(E, Et, Nn, Nt, n);
  for (int k = 0; k < kAnSets; ++k) slots += an_pow2_slots(n[k]);
  return 256 + 256 + (size_t)slots * sizeof(int);  // alignment slack, the counts, the sets
}

extern "C" int tgmx_batch_analytics(const tgmx_an_batch_t* batch, int32_t time_as_f32, int64_t* out, void* workspace, size_t workspace_bytes,
                                    tgmx_stream_t stream) {
  TGMX_REQUIRE(batch && out && workspace, "batch_analytics: null pointer");
  const tgmx_an_batch_t& b = *batch;
  TGMX_REQUIRE(ba_sizes_ok(b.E, b.Et, b.Nn, b.Nt), "batch_analytics: bad sizes E=%lld Et=%lld Nn=%lld Nt=%lld", (long long)b.E, (long long)b.Et,
               (long long)b.Nn, (long long)b.Nt);
  TGMX_REQUIRE((b.E == 0 || (b.src && b.dst)) && (b.Et == 0 || b.edge_time) && (b.Nn == 0 || b.nids) && (b.Nt == 0 || b.node_time),
               "batch_analytics: a field with a count has no pointer");
  const size_t need = tgmx_batch_analytics_workspace_bytes(b.E, b.Et, b.Nn, b.Nt);
  TGMX_REQUIRE(workspace_bytes >= need, "batch_analytics: workspace too small (%zu of %zu bytes)", workspace_bytes, need);
  BaArgs a{};
  a.b = b;
  a.time_as_f32 = time_as_f32 != 0;
  ba_set_sizes(b.E, b.Et, b.Nn, b.Nt, a.n);
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  a.counts = reinterpret_cast<unsigned long long*>(base);
  int* slots = reinterpret_cast<int*>(base + 256);
  long long item = 0, slot = 0;
  for (int k = 0; k < kAnSets; ++k) {
    const long long cap = an_pow2_slots(a.n[k]);
    a.first[k] = item;
    a.slots[k] = slots + slot;
    a.mask[k] = (unsigned)(cap - 1);
    item += a.n[k];
    slot += cap;
  }
  a.total = item;
  a.slots_total = slot;
  a.out = out;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ba_reset_kernel, dim3(eb_grid(slot)), dim3(kAnThreads), 0, st, a);
  TGMX_CHECK_LAUNCH("batch_analytics(reset)");
  if (a.total > 0) {
    hipLaunchKernelGGL(ba_insert_kernel, dim3(eb_grid(a.total)), dim3(kAnThreads), 0, st, a);
    TGMX_CHECK_LAUNCH("batch_analytics(insert)");
  }
  hipLaunchKernelGGL(ba_finish_kernel, dim3(1), dim3(kWave), 0, st, a);
  TGMX_CHECK_LAUNCH("batch_analytics(finish)");
  return TGMX_OK;
}

extern "C" int tgmx_seen_nodes_step(uint8_t* mask, int64_t num_nodes, const void* src, int32_t src_is64, const void* dst, int32_t dst_is64, int64_t E,
                                    const void* nids, int32_t nids_is64, int64_t Ny, int64_t* out_pos, void* out_ids, int64_t* state,
                                    tgmx_stream_t stream) {
  TGMX_REQUIRE(num_nodes >= 0 && E >= 0 && Ny >= 0 && E < (1ll << 40) && state, "seen_nodes_step: bad sizes or null state");
  TGMX_REQUIRE((num_nodes == 0 || mask) && (E == 0 || (src && dst)) && (Ny == 0 || (nids && out_pos && out_ids)), "seen_nodes_step: null pointer");
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* status = reinterpret_cast<unsigned long long*>(state + 1);
  if (E > 0) {
    hipLaunchKernelGGL(sn_mark_kernel, dim3(eb_grid(2 * E)), dim3(kAnThreads), 0, st, mask, (long long)num_nodes, src, (int)(src_is64 != 0), dst,
                       (int)(dst_is64 != 0), (long long)E, status);
    TGMX_CHECK_LAUNCH("seen_nodes_step(mark)");
  }
  if (Ny > 0) {
    hipLaunchKernelGGL(sn_compact_kernel, dim3(1), dim3(kSnThreads), 0, st, (const uint8_t*)mask, (long long)num_nodes, nids, (int)(nids_is64 != 0),
                       (long long)Ny, out_pos, out_ids, reinterpret_cast<long long*>(state), status);
    TGMX_CHECK_LAUNCH("seen_nodes_step(compact)");
  }
  return TGMX_OK;
}

extern "C" int tgmx_node_analytics_step(const tgmx_node_analytics_t* st_, const tgmx_an_batch_t* batch, int64_t call, int64_t* out,
                                        tgmx_stream_t stream) {
  TGMX_REQUIRE(st_ && batch && out, "node_analytics_step: null pointer");
  const tgmx_node_analytics_t& s = *st_;
  const tgmx_an_batch_t& b = *batch;
  TGMX_REQUIRE(s.slot_of && s.first_seen && s.last_seen && s.appearances && s.edges && s.nbrs && s.times && s.apps && s.counters && s.degree &&
                   s.new_nbrs && s.present && s.stamp && s.scalars,
               "node_analytics_step: null state pointer");
  TGMX_REQUIRE(s.num_nodes > 0 && s.num_nodes < (1ll << 31) && s.T >= 0 && s.T <= s.num_nodes, "node_analytics_step: bad sizes N=%lld T=%lld",
               (long long)s.num_nodes, (long long)s.T);
  TGMX_REQUIRE(an_pow2(s.edges_cap) && an_pow2(s.nbrs_cap) && an_pow2(s.times_cap) && an_pow2(s.apps_cap), "node_analytics_step: capacities must be powers of two");
  TGMX_REQUIRE(call > 0 && call < (1ll << 31), "node_analytics_step: call %lld", (long long)call);
  const long long lim = 1ll << 40;
  TGMX_REQUIRE(b.E >= 0 && b.E < lim && b.Nn >= 0 && b.Nn < lim && b.Et >= 0 && b.Et < lim && b.Nt >= 0 && b.Nt < lim, "node_analytics_step: bad batch sizes");
  TGMX_REQUIRE((b.E == 0 || (b.src && b.dst)) && (b.Et == 0 || b.edge_time) && (b.Nn == 0 || b.nids) && (b.Nt == 0 || b.node_time),
               "node_analytics_step: a field with a count has no pointer");
  NaArgs a{s, b, (long long)call, out};
  hipStream_t st = (hipStream_t)stream;
  if (b.Et + b.Nt > 0) {
    hipLaunchKernelGGL(na_time_kernel, dim3(eb_grid(b.Et + b.Nt)), dim3(kAnThreads), 0, st, a);
    TGMX_CHECK_LAUNCH("node_analytics_step(times)");
  }
  if (b.E + b.Nn > 0) {
    hipLaunchKernelGGL(na_event_kernel, dim3(eb_grid(b.E + b.Nn)), dim3(kAnThreads), 0, st, a);
    TGMX_CHECK_LAUNCH("node_analytics_step(events)");
  }
  hipLaunchKernelGGL(na_finalise_kernel, dim3(eb_grid(s.T + 2)), dim3(kAnThreads), 0, st, a);
  TGMX_CHECK_LAUNCH("node_analytics_step(finalise)");
  return TGMX_OK;
}

extern "C" int tgmx_node_analytics_rehash(const void* from, int64_t from_cap, void* to, int64_t to_cap, int64_t* state, tgmx_stream_t stream) {
  TGMX_REQUIRE(from && to && state && an_pow2(from_cap) && an_pow2(to_cap), "node_analytics_rehash: null pointer or a capacity that is no power of two");
  hipLaunchKernelGGL(na_rehash_kernel, dim3(eb_grid(from_cap)), dim3(kEbThreads), 0, (hipStream_t)stream, static_cast<const EbSlot*>(from),
                     (long long)from_cap, static_cast<EbSlot*>(to), (long long)to_cap, state);
  TGMX_CHECK_LAUNCH("node_analytics_rehash");
  return TGMX_OK;
}
