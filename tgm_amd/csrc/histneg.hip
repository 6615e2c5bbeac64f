// HistoricalNegativeEdgeSamplerHook (the reference's tgm/hooks/negatives/sampler.py:68-238), for gfx950: per batch position one uniformly drawn
// past destination of its source, and the append of the batch to the per-source histories.  The reference re-reads its whole event log per
// batch (isin, unique, a rand per matching event, scatter-max); here a draw is O(1) expected loads and an appended event O(1) stores.
//
// History of a source: its past destinations in arrival order, as a chain of segments in one int32 pool.  Segment k holds 4 * 2^k
// destinations, the ranks [4 (2^k - 1), 4 (2^(k+1) - 1)), behind a ONE-word header with the pool offset of segment k - 1 (-1 for k = 0).
// Rank r lives in segment seg(r) = floor(log2(r / 4 + 1)) (one clz).  tail[s] is the offset of s's newest segment, whose k is seg(cnt[s] - 1);
// a reader follows seg(cnt - 1) - seg(r) back links and indexes.  Half of all ranks sit in the newest segment, so a uniform draw follows
// less than one link on average (sum_j j 2^-(j+1) < 1) and at most log2(cnt) in the worst case.  Segments are handed out by atomicAdd on a
// device-side bump pointer and never move: offsets are pool-relative, so the caller may copy the pool into a larger one.
//
// Pool bound.  A source with n >= 1 events owns the segments 0..K, K = seg(n - 1), so 4 (2^K - 1) <= n - 1, i.e. 2^K <= (n + 3) / 4:
//   slots   = 4 (2^(K+1) - 1) = 8 2^K - 4 <= 2 n + 2
//   headers = K + 1 <= 2^K <= (n + 3) / 4
// so at most 2.25 n + 2.75 words; summed over the at most min(count, N) sources that have events:
//   words <= (9 count + 11 min(count, N)) / 4                                                                        (the caller adds 1)
// The caller grows the pool from this bound BEFORE a call that could pass it; pool_top is never read on the path.  The kernels still check
// every offset against pool_cap (status bit 2), so a pool that is too small loses events instead of writing outside it.
//
// Append order.  Same-source events of a batch must take consecutive ranks in batch order (the draws are defined over the arrival order).
// The batch is grouped by ONE stable radix sort of (source id, position) -- rocPRIM's, as the CSR builds of cheb.hip / gcn.hip use it --
// and ranks follow from the sorted position: rank = cnt_before + (t - first t of the group).  Per group the leader (first sorted position)
// allocates ALL segments the group needs with one atomicAdd, links them (at most log2 of the group's size header stores) and advances cnt /
// tail; a launch boundary later every event stores its own destination.  A batch of B events of one source is one leader doing O(log B)
// stores and B lanes storing in parallel.  Nothing depends on scheduling but the segments' positions in the pool.
#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

namespace tgmx {

constexpr int kHnBadId = 1, kHnOverflow = 2;  // status bits
constexpr int kHnThreads = 256;

__device__ __forceinline__ int hn_seg(int r) { return 31 - __clz((r >> 2) + 1); }     // r >= 0
__device__ __forceinline__ int hn_seg_first(int k) { return 4 * ((1 << k) - 1); }    // first rank of segment k

// pool index of rank r of a source with n > r events and newest segment at `tail`; -1: the chain leaves the pool
__device__ __forceinline__ long long hn_slot(const int* pool, long long cap, int tail, int n, int r) {
  const int kr = hn_seg(r);
  long long off = tail;
  for (int h = hn_seg(n - 1) - kr; h > 0; --h) {
    if (off < 0 || off >= cap) return -1;
    off = pool[off];
  }
  const long long idx = off + 1 + (r - hn_seg_first(kr));
  return (off < 0 || idx >= cap) ? -1 : idx;
}

struct HnArgs {
  int* cnt;
  int* tail;
  long long N;
  int* pool;
  long long pool_cap;
  int* state;  // {pool_top, status}
  int* memory;
  long long mem_cap, count;
  unsigned long long seed, call;
  const void *src, *dst;
  int src64, dst64;
  const int64_t* time;
  long long B;
  int* neg;
  int64_t* neg_time;
  uint8_t* valid;
  unsigned *key_in, *key, *pos_in, *pos;  // the sort's input and output
  int* gbase;                             // [B], at a group's first sorted position: cnt before the batch (-1: the group was dropped)
};

__device__ __forceinline__ long long hn_grid_start() { return (long long)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ long long hn_grid_step() { return (long long)gridDim.x * blockDim.x; }

// (a): the draw from the state before this batch, the log, the sort's keys
__global__ __launch_bounds__(kHnThreads) void hn_sample_kernel(HnArgs a) {
  for (long long i = hn_grid_start(); i < a.B; i += hn_grid_step()) {
    const long long s = ld_idx(a.src, a.src64, i), d = ld_idx(a.dst, a.dst64, i);
    const bool ok = s >= 0 && s < a.N;
    a.memory[a.count + i] = (int)s;
    a.memory[a.mem_cap + a.count + i] = (int)d;
    a.key_in[i] = ok ? (unsigned)s : (unsigned)a.N;  // out-of-range ids sort behind every node
    a.pos_in[i] = (unsigned)i;
    if (a.neg_time) a.neg_time[i] = a.time[i];
    if (!ok) atomicOr(&a.state[1], kHnBadId);
    if (!a.neg) continue;
    int out = -1;
    const int n = ok ? a.cnt[s] : 0;
    if (n > 0) {
      const int r = (int)__umulhi(counter_u32(a.seed, a.call, (unsigned long long)s), (unsigned)n);
      const long long idx = hn_slot(a.pool, a.pool_cap, a.tail[s], n, r);
      if (idx >= 0) out = a.pool[idx];
      else atomicOr(&a.state[1], kHnOverflow);
    }
    a.neg[i] = out;
    a.valid[i] = out != -1;
  }
}

// (b) 1: one lane per group
__global__ __launch_bounds__(kHnThreads) void hn_leader_kernel(HnArgs a) {
  for (long long t = hn_grid_start(); t < a.B; t += hn_grid_step()) {
    const unsigned key = a.key[t];
    if ((long long)key >= a.N || (t > 0 && a.key[t - 1] == key)) continue;
    long long lo = t + 1, hi = a.B;  // the group's end: the first position behind t with another key
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (a.key[mid] == key) lo = mid + 1;
      else hi = mid;
    }
    const int g = (int)(lo - t), n = a.cnt[key];
    const int k_old = n > 0 ? hn_seg(n - 1) : -1, k_new = hn_seg(n + g - 1);
    int base = n;
    if (k_new > k_old) {
      // the segments k_old + 1 .. k_new: their headers and 4 (2^(k_new + 1) - 2^(k_old + 1)) slots
      const long long words = (long long)(k_new - k_old) + 4ll * ((1ll << (k_new + 1)) - (1ll << (k_old + 1)));
      long long off = -1;
      if (words <= a.pool_cap) {
        off = atomicAdd(&a.state[0], (int)words);
        if (off < 0 || off + words > a.pool_cap) off = -1;
      }
      if (off < 0) {
        atomicOr(&a.state[1], kHnOverflow);
        base = -1;
      } else {
        int prev = n > 0 ? a.tail[key] : -1;
        for (int k = k_old + 1; k <= k_new; ++k) {
          a.pool[off] = prev;
          prev = (int)off;
          off += 1 + (4ll << k);
        }
        a.tail[key] = prev;
      }
    }
    if (base >= 0) a.cnt[key] = n + g;
    a.gbase[t] = base;
  }
}

// (b) 2: one lane per event
__global__ __launch_bounds__(kHnThreads) void hn_member_kernel(HnArgs a) {
  for (long long t = hn_grid_start(); t < a.B; t += hn_grid_step()) {
    const unsigned key = a.key[t];
    if ((long long)key >= a.N) continue;
    long long lo = 0, hi = t;  // the group's first position
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (a.key[mid] < key) lo = mid + 1;
      else hi = mid;
    }
    const int base = a.gbase[lo];
    if (base < 0) continue;
    const long long idx = hn_slot(a.pool, a.pool_cap, a.tail[key], a.cnt[key], base + (int)(t - lo));
    if (idx >= 0) a.pool[idx] = a.memory[a.mem_cap + a.count + a.pos[t]];
    else atomicOr(&a.state[1], kHnOverflow);
  }
}

struct HnLayout {
  size_t key_in, key, pos_in, pos, gbase, temp, temp_bytes, total;
};
static int hn_layout(long long B, HnLayout& w) {
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t n = (size_t)(B > 0 ? B : 1);
  size_t off = 0;
  w.key_in = off; off = up(off + n * 4);
  w.key = off; off = up(off + n * 4);
  w.pos_in = off; off = up(off + n * 4);
  w.pos = off; off = up(off + n * 4);
  w.gbase = off; off = up(off + n * 4);
  size_t tb = 0;
  if (rocprim::radix_sort_pairs(nullptr, tb, (const unsigned*)nullptr, (unsigned*)nullptr, (const unsigned*)nullptr, (unsigned*)nullptr, n, 0u, 32u) !=
      hipSuccess)
    return TGMX_E_LAUNCH;
  w.temp = off; w.temp_bytes = tb; off = up(off + tb);
  w.total = off + 256;
  return TGMX_OK;
}

}  // namespace tgmx

using namespace tgmx;

extern "C" size_t tgmx_histneg_workspace_bytes(int64_t B, int64_t num_nodes) {
  HnLayout w;
  if (B < 0 || B >= (1ll << 31) || num_nodes <= 0 || num_nodes >= (1ll << 31)) return 0;
  return hn_layout(B, w) == TGMX_OK ? w.total : 0;
}

extern "C" int tgmx_histneg_step(const tgmx_histneg_t* h, const void* src, int32_t src_is64, const void* dst, int32_t dst_is64, const int64_t* time,
                                 int64_t B, int32_t* neg, int64_t* neg_time, uint8_t* valid, void* workspace, size_t workspace_bytes,
                                 tgmx_stream_t stream) {
  TGMX_REQUIRE(h && h->cnt && h->tail && h->pool && h->state && h->memory, "histneg_step: null state pointer");
  TGMX_REQUIRE(h->num_nodes > 0 && h->num_nodes < (1ll << 31) && h->pool_cap > 0 && h->pool_cap < (1ll << 31), "histneg_step: bad sizes N=%lld pool=%lld",
               (long long)h->num_nodes, (long long)h->pool_cap);
  TGMX_REQUIRE(B >= 0 && h->count >= 0 && h->count + B <= h->mem_cap && h->count + B < (1ll << 31),
               "histneg_step: the log holds %lld events, %lld + %lld offered", (long long)h->mem_cap, (long long)h->count, (long long)B);
  if (B == 0) return TGMX_OK;
  TGMX_REQUIRE(src && dst && workspace, "histneg_step: null pointer");
  TGMX_REQUIRE((neg == nullptr) == (valid == nullptr) && (time == nullptr) == (neg_time == nullptr), "histneg_step: neg / valid and time / neg_time go together");
  HnLayout l;
  if (hn_layout(B, l) != TGMX_OK || workspace_bytes < l.total) {
    set_error("histneg_step: workspace too small (%zu bytes)", workspace_bytes);
    return TGMX_E_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  HnArgs a{h->cnt, h->tail, (long long)h->num_nodes, h->pool, (long long)h->pool_cap, h->state, h->memory, (long long)h->mem_cap, (long long)h->count,
           h->seed, h->call, src, dst, src_is64 != 0, dst_is64 != 0, time, (long long)B, neg, neg_time, valid,
           reinterpret_cast<unsigned*>(base + l.key_in), reinterpret_cast<unsigned*>(base + l.key), reinterpret_cast<unsigned*>(base + l.pos_in),
           reinterpret_cast<unsigned*>(base + l.pos), reinterpret_cast<int*>(base + l.gbase)};
  const long long blocks = (B + kHnThreads - 1) / kHnThreads;
  const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096)), block(kHnThreads);
  hipLaunchKernelGGL(hn_sample_kernel, grid, block, 0, st, a);
  TGMX_CHECK_LAUNCH("histneg_step(sample)");
  int sb = 1;
  while ((1ll << sb) <= h->num_nodes) ++sb;  // the keys go up to num_nodes itself (the out-of-range ids)
  size_t tb = l.temp_bytes;
  if (rocprim::radix_sort_pairs(base + l.temp, tb, (const unsigned*)a.key_in, a.key, (const unsigned*)a.pos_in, a.pos, (size_t)B, 0u, (unsigned)sb, st) !=
      hipSuccess) {
    set_error("histneg_step: radix sort failed");
    return TGMX_E_LAUNCH;
  }
  hipLaunchKernelGGL(hn_leader_kernel, grid, block, 0, st, a);
  TGMX_CHECK_LAUNCH("histneg_step(leaders)");
  hipLaunchKernelGGL(hn_member_kernel, grid, block, 0, st, a);
  TGMX_CHECK_LAUNCH("histneg_step(members)");
  return TGMX_OK;
}
