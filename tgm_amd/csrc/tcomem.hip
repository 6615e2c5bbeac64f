// tCoMemPredictor (the reference's tgm/nn/modules/t_comem.py), for gfx950: the per-node ring of recent events, the popularity counts and the
// pair counts on the device, the batch update, the batched queries (flat, and one source against its destination and its negatives) and the
// rehash of the pair counts into a larger table.
//
// State: per node a ring row of k entries {float32 ts, int32 dst} (a k = 50 row is 400 contiguous bytes) with int32 pos and len; an int32
// popularity count per node, converted to float32 where it is read (exact below 2^24); the pair counter, the table of pairtable.h with
// key = min(s, d) << 32 | max(s, d) and the count as the value: the reference increments [s][d] and [d][s] together, so one counter per
// unordered pair holds both, and a self-loop adds 2; a 16-byte state block {int64 end, float32 size}.
//
// Update: one workgroup, one event per thread, up to 1024 events a launch; a longer call is cut into launches of 1024 in arrival order, which
// leaves what one pass over all of it would leave (every phase below is a sum, a maximum, or the sequential ring rule applied to a prefix).
//   1  every valid event finds or claims its pair's slot and adds to the count; popularity[dst] += 1 (integer atomics)
//   2  max(ts) -> end
//   3  every event counts, over the sources in LDS, its rank among the launch's events of its source (arrival order) and their number cnt;
//      event `rank` writes ring slot (pos0 + rank) % k iff rank >= cnt - k (what sequential overwriting leaves), and the event with
//      rank == cnt - 1 writes pos = (pos0 + cnt) % k, len = min(len0 + cnt, k).  A barrier separates the reads of pos0 / len0 from that write.
// No float takes part in an atomic and every ring slot, pos and len has exactly one writer per launch: two runs leave the same ring, pos, len,
// popularity and counts (the slot positions in the table may differ with the order in which colliding keys claim).
//
// Query: one wave per row (the flat form is rows of one candidate).  The wave reduces the source's base score once, in one routine with one
// fixed order (lane l adds its entries l, l + 64, .. in turn, then an xor butterfly), so a source's base score has the same bits wherever it
// is computed; its lanes then probe the pair table for the row's candidates.
#include "pairtable.h"

namespace tgmx {

constexpr int kTcBadId = 1, kTcOverflow = 2, kTcBadSrc = 4, kTcBadDst = 8;  // status bits
constexpr int kTcBlockMax = 1024;                                           // events one update launch takes

struct TcEntry {
  float ts;
  int dst;
};
struct alignas(16) TcState {  // tgmx_tcomem_state_bytes()
  long long end;              // the largest timestamp seen
  float size;                 // the window size, float32 as the reference's 0-dim tensor
  int pad_;
};
static_assert(sizeof(TcState) == 16 && sizeof(TcEntry) == 8, "tcomem layouts");

struct TcArgs {  // tgmx_tcomem_t, typed
  TcEntry* ring;
  int *pos, *len, *pop;
  EbSlot* table;
  long long cap;
  TcState* state;
  long long N;
  int k;
  double weight;
  int* status;
};

__device__ __forceinline__ unsigned long long tc_key(long long s, long long d) {
  return s < d ? ((unsigned long long)s << 32) | (unsigned long long)d : ((unsigned long long)d << 32) | (unsigned long long)s;
}

struct TcUpdateArgs {
  const void *src, *dst, *ts;
  int src64, dst64, ts64;
  long long first;  // the launch's first event
  int n;            // its events, <= kTcBlockMax
};

__global__ __launch_bounds__(kTcBlockMax) void tc_update_kernel(TcArgs a, TcUpdateArgs u) {
  __shared__ __attribute__((aligned(16))) int s_src[kTcBlockMax];
  __shared__ long long s_max[kTcBlockMax / kWave];
  const int tid = threadIdx.x;
  long long s = -1, d = -1, t = 0;
  bool live = false;
  if (tid < u.n) {
    s = ld_idx(u.src, u.src64, u.first + tid);
    d = ld_idx(u.dst, u.dst64, u.first + tid);
    t = ld_idx(u.ts, u.ts64, u.first + tid);
    int bad = 0;
    if (!eb_id_ok(s, d)) bad = kTcBadId;
    else bad = (s >= a.N ? kTcBadSrc : 0) | (d >= a.N ? kTcBadDst : 0);
    if (!bad) {
      const long long slot = eb_claim(a.table, a.cap, tc_key(s, d));
      if (slot < 0) bad = kTcOverflow;
      else atomicAdd(reinterpret_cast<unsigned long long*>(a.table) + 2 * slot + 1, s == d ? 2ull : 1ull);
    }
    if (bad) atomicOr(a.status, bad);  // the event contributes nothing
    else live = true;
  }
  int pos0 = 0, len0 = 0;
  if (live) {
    atomicAdd(&a.pop[d], 1);
    pos0 = a.pos[s];
    len0 = a.len[s];
  }
  s_src[tid] = live ? (int)s : -1;
  long long m = live ? t : INT64_MIN;
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const long long o = __shfl_xor(m, off);
    m = o > m ? o : m;
  }
  if (lane_id() == 0) s_max[tid / kWave] = m;
  __syncthreads();  // s_src and s_max are whole; every read of pos / len above precedes the writes below
  if (tid == 0) {
    long long end = a.state->end;
    for (int w = 0; w < (int)(blockDim.x / kWave); ++w) end = s_max[w] > end ? s_max[w] : end;
    a.state->end = end;
  }
  if (!live) return;
  int rank = 0, cnt = 0;
  const int me = (int)s;
  for (int j = 0; j < (int)blockDim.x; j += 4) {  // blockDim.x is a multiple of the wave; every lane reads the same 16 bytes (a broadcast)
    const int4 v = *reinterpret_cast<const int4*>(&s_src[j]);
    const int e0 = v.x == me, e1 = v.y == me, e2 = v.z == me, e3 = v.w == me;
    cnt += e0 + e1 + e2 + e3;
    rank += (e0 & (j < tid)) + (e1 & (j + 1 < tid)) + (e2 & (j + 2 < tid)) + (e3 & (j + 3 < tid));
  }
  if (rank >= cnt - a.k) a.ring[s * a.k + (pos0 + rank) % a.k] = TcEntry{(float)t, (int)d};  // the timestamp is rounded to float32 here
  if (rank == cnt - 1) {
    a.pos[s] = (pos0 + cnt) % a.k;
    a.len[s] = len0 + cnt < a.k ? len0 + cnt : a.k;
  }
}

struct TcQueryArgs {
  const void *src, *dst, *neg;
  int src64, dst64, neg64;
  const int64_t* neg_off;  // [B + 1] for ragged rows, NULL: M per row
  long long M, B, total;
  float* out;
  int dtype;  // the dtype of the query's ids: 0 int32, 1 int64, 2 float32, 3 float64
};

// The base score of source s, on every lane of the wave: the sum over ring entries i < len with start <= ts <= f32(end) of
// exp(-(f32(end) - ts) / size) * sigmoid(popularity[dst]), all float32.  Accurate expf and division; the products and sums are kept apart
// (no contraction), so the value depends on nothing but the state.
__device__ __forceinline__ float tc_base(const TcArgs& a, long long s, float endf, float start, float size) {
  const int len = a.len[s];
  const TcEntry* row = a.ring + s * a.k;
  float acc = 0.0f;
  for (int i = lane_id(); i < a.k; i += kWave) {
    if (i >= len) continue;
    const float2 raw = *reinterpret_cast<const float2*>(&row[i]);  // one 8-byte load
    const float ts = raw.x;
    const int dst = __float_as_int(raw.y);
    if (!(ts >= start && ts <= endf) || (unsigned)dst >= (unsigned long long)a.N) continue;
    const float decay = expf(-(endf - ts) / size);
    const float pop = 1.0f / (1.0f + expf(-(float)a.pop[dst]));
    acc = __fadd_rn(acc, __fmul_rn(decay, pop));
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, off));  // a + b on one lane, b + a on its partner
  return acc;
}

__global__ __launch_bounds__(kEbThreads) void tc_query_kernel(TcArgs a, TcQueryArgs q) {
  const TcState st = *a.state;
  const float endf = (float)st.end, size = st.size;
  const float start = endf - size;
  const long long waves = (long long)gridDim.x * (kEbThreads / kWave);
  const long long negs = q.total - q.B;  // entries of neg[]
  for (long long b = (long long)blockIdx.x * (kEbThreads / kWave) + threadIdx.x / kWave; b < q.B; b += waves) {
    const long long s = ld_idx(q.src, q.src64, b);
    long long nbase = 0, obase = b, cnt = 1;  // flat: row b is the one pair (src[b], dst[b])
    if (q.neg) {                               // one against many: (src[b], dst[b]) then (src[b], neg[b][m])
      if (q.neg_off) {
        nbase = (long long)q.neg_off[b];
        cnt = (long long)q.neg_off[b + 1] - nbase + 1;
        obase = nbase + b;
      } else {
        nbase = b * q.M;
        cnt = q.M + 1;
        obase = b * (q.M + 1);
      }
    }
    const bool src_ok = s >= 0 && s < a.N;
    if (!src_ok && lane_id() == 0) atomicOr(a.status, s >= 0 && s < (1ll << 31) ? kTcBadSrc : kTcBadId);
    const float base = src_ok ? tc_base(a, s, endf, start, size) : 0.0f;  // (the branch is the wave's)
    for (long long c = lane_id(); c < cnt; c += kWave) {
      if (nbase < 0 || obase + c >= q.total || (c > 0 && nbase + c - 1 >= negs)) break;  // offsets that do not describe `total` answers
      const long long d = c == 0 ? ld_idx(q.dst, q.dst64, b) : ld_idx(q.neg, q.neg64, nbase + c - 1);
      float v = 0.0f;
      if (d < 0 || d >= (1ll << 31)) {
        atomicOr(a.status, kTcBadId);
      } else if (src_ok) {
        v = base;
        long long co = 0;
        if (q.dtype >= 2 && eb_find(a.table, a.cap, tc_key(s, d), &co) >= 0 && co > 0) {
          // the reference's Python: weight * (c / (1 + c)) in doubles, stored into zeros_like(query_src)
          const double term = a.weight * ((double)co / (1.0 + (double)co));
          v = q.dtype == 2 ? __fadd_rn(base, (float)term) : (float)((double)base + term);
        }
      }
      q.out[obase + c] = v;
    }
  }
}

struct TcRehashArgs {
  const EbSlot* from;
  long long from_cap;
  EbSlot* to;
  long long to_cap;
  int* status;
  unsigned long long* kept;
};

// every pair moves: counts never leave
__global__ __launch_bounds__(kEbThreads) void tc_rehash_kernel(TcRehashArgs a) {
  eb_move_slots(a.from, a.from_cap, a.to, a.to_cap, a.status, kTcOverflow, a.kept, [](long long) { return true; });
}

static bool tc_valid(const tgmx_tcomem_t* tc) {
  return tc && tc->ring && tc->pos && tc->len && tc->popularity && tc->table && tc->state && tc->status && tc->capacity >= 2 &&
         tc->capacity < (1ll << 40) && (tc->capacity & (tc->capacity - 1)) == 0 && tc->num_nodes > 0 && tc->num_nodes <= (1ll << 31) && tc->k > 0 &&
         tc->k <= tc->num_nodes;
}
static TcArgs tc_args(const tgmx_tcomem_t* tc) {
  return TcArgs{reinterpret_cast<TcEntry*>(tc->ring), tc->pos, tc->len, tc->popularity, reinterpret_cast<EbSlot*>(tc->table), (long long)tc->capacity,
                reinterpret_cast<TcState*>(tc->state), (long long)tc->num_nodes, tc->k, tc->co_occurrence_weight, tc->status};
}

}  // namespace tgmx

using namespace tgmx;

extern "C" size_t tgmx_tcomem_state_bytes(void) { return sizeof(TcState); }

extern "C" int tgmx_tcomem_update(const tgmx_tcomem_t* tc, const void* src, int32_t src_is64, const void* dst, int32_t dst_is64, const void* ts,
                                  int32_t ts_is64, int64_t n, tgmx_stream_t stream) {
  TGMX_REQUIRE(tc_valid(tc), "tcomem_update: bad state block (capacity a power of two >= 2, 0 < k <= num_nodes <= 2^31)");
  TGMX_REQUIRE(n >= 0, "tcomem_update: bad size n=%lld", (long long)n);
  if (n == 0) return TGMX_OK;
  TGMX_REQUIRE(src && dst && ts, "tcomem_update: null pointer");
  const TcArgs a = tc_args(tc);
  for (long long first = 0; first < n; first += kTcBlockMax) {
    const int m = (int)(n - first < kTcBlockMax ? n - first : kTcBlockMax);
    TcUpdateArgs u{src, dst, ts, src_is64 != 0, dst_is64 != 0, ts_is64 != 0, first, m};
    hipLaunchKernelGGL(tc_update_kernel, dim3(1), dim3((unsigned)((m + kWave - 1) / kWave * kWave)), 0, (hipStream_t)stream, a, u);
    TGMX_CHECK_LAUNCH("tcomem_update");
  }
  return TGMX_OK;
}

extern "C" int tgmx_tcomem_query(const tgmx_tcomem_t* tc, const void* src, int32_t src_is64, const void* dst, int32_t dst_is64, const void* neg,
                                 int32_t neg_is64, const int64_t* neg_off, int64_t M, int64_t B, int64_t total, float* out, int32_t query_dtype,
                                 tgmx_stream_t stream) {
  TGMX_REQUIRE(tc_valid(tc), "tcomem_query: bad state block (capacity a power of two >= 2, 0 < k <= num_nodes <= 2^31)");
  TGMX_REQUIRE(B >= 0 && total >= 0 && M >= 0 && query_dtype >= 0 && query_dtype <= 3, "tcomem_query: bad sizes B=%lld total=%lld M=%lld query_dtype=%d",
               (long long)B, (long long)total, (long long)M, query_dtype);
  TGMX_REQUIRE(neg || neg_off || total == B, "tcomem_query: the flat form answers one query per pair (total=%lld, B=%lld)", (long long)total, (long long)B);
  TGMX_REQUIRE(!neg || neg_off || total == B * (M + 1), "tcomem_query: [B, M] negatives give B (M + 1) answers (total=%lld)", (long long)total);
  TGMX_REQUIRE(!neg_off || (neg && total >= B), "tcomem_query: row offsets without negatives, or fewer answers than rows");
  if (total == 0) return TGMX_OK;
  TGMX_REQUIRE(src && dst && out && B > 0, "tcomem_query: null pointer");
  TcQueryArgs q{src, dst, neg, src_is64 != 0, dst_is64 != 0, neg_is64 != 0, neg_off, (long long)M, (long long)B, (long long)total, out, query_dtype};
  hipLaunchKernelGGL(tc_query_kernel, dim3(eb_grid(B * kWave)), dim3(kEbThreads), 0, (hipStream_t)stream, tc_args(tc), q);
  TGMX_CHECK_LAUNCH("tcomem_query");
  return TGMX_OK;
}

extern "C" int tgmx_tcomem_rehash(const tgmx_tcomem_t* from, const tgmx_tcomem_t* to, int64_t* kept, tgmx_stream_t stream) {
  TGMX_REQUIRE(tc_valid(from) && tc_valid(to) && kept, "tcomem_rehash: bad state block");
  TGMX_REQUIRE(to->capacity >= 2 * from->capacity && to->table != from->table, "tcomem_rehash: the new table must be at least twice the old (%lld -> %lld)",
               (long long)from->capacity, (long long)to->capacity);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(kept, 0, sizeof(int64_t), st) != hipSuccess) {
    set_error("tcomem_rehash: clearing the count failed");
    return TGMX_E_LAUNCH;
  }
  TcRehashArgs a{reinterpret_cast<const EbSlot*>(from->table), (long long)from->capacity, reinterpret_cast<EbSlot*>(to->table), (long long)to->capacity,
                 to->status, reinterpret_cast<unsigned long long*>(kept)};
  hipLaunchKernelGGL(tc_rehash_kernel, dim3(eb_grid(from->capacity)), dim3(kEbThreads), 0, st, a);
  TGMX_CHECK_LAUNCH("tcomem_rehash");
  return TGMX_OK;
}
