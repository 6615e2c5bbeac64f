// The pair table edgebank.hip and tcomem.hip share: open addressing, linear probing, capacity a power of two.  A slot is 16 bytes
// {uint64 key, int64 value}, so a probe is one 16-byte load; the empty key is all ones (ids lie in [0, 2^31), so no pair packs to it).  A
// key is written once, by a 64-bit compare-and-swap, and never changes or leaves until a rehash: a probe that meets an empty slot has seen
// every slot the key could be in.  Every probe loop is a for over at most `capacity` probes.
#pragma once

#include "common.h"

namespace tgmx {

constexpr unsigned long long kEbEmpty = ~0ull;
constexpr int kEbThreads = 256;

struct EbSlot {
  unsigned long long key;
  long long val;  // EdgeBank: the pair's timestamp; t-CoMem: the pair's count
};
static_assert(sizeof(EbSlot) == 16, "pair table slot");

__device__ __forceinline__ unsigned long long eb_hash(unsigned long long x) {  // the splitmix64 finaliser
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ bool eb_id_ok(long long s, long long d) { return s >= 0 && s < (1ll << 31) && d >= 0 && d < (1ll << 31); }

// slot of `key`, claimed if absent; -1 when `cap` probes found neither the key nor room
__device__ __forceinline__ long long eb_claim(EbSlot* __restrict__ table, long long cap, unsigned long long key) {
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(table);
  long long i = (long long)(eb_hash(key) & (unsigned long long)(cap - 1));
  for (long long p = 0; p < cap; ++p) {
    unsigned long long cur = __hip_atomic_load(&keys[2 * i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kEbEmpty) cur = atomicCAS(&keys[2 * i], kEbEmpty, key);  // returns what was there: empty (now mine), mine, or another's
    if (cur == kEbEmpty || cur == key) return i;
    i = (i + 1) & (cap - 1);
  }
  return -1;
}
// eb_claim that also tells whether THIS call took the slot (*fresh: the compare-and-swap returned the empty key): of all the claims of one
// key, in one launch or over many, exactly one is fresh
__device__ __forceinline__ long long eb_claim_fresh(EbSlot* __restrict__ table, long long cap, unsigned long long key, bool* fresh) {
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(table);
  long long i = (long long)(eb_hash(key) & (unsigned long long)(cap - 1));
  *fresh = false;
  for (long long p = 0; p < cap; ++p) {
    unsigned long long cur = __hip_atomic_load(&keys[2 * i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kEbEmpty) {
      cur = atomicCAS(&keys[2 * i], kEbEmpty, key);
      if (cur == kEbEmpty) {
        *fresh = true;
        return i;
      }
    }
    if (cur == key) return i;
    i = (i + 1) & (cap - 1);
  }
  return -1;
}
// slot of `key`, or -1 (absent: an empty slot ends the probe)
__device__ __forceinline__ long long eb_find(const EbSlot* __restrict__ table, long long cap, unsigned long long key, long long* val_out) {
  long long i = (long long)(eb_hash(key) & (unsigned long long)(cap - 1));
  for (long long p = 0; p < cap; ++p) {
    const ulonglong2 s = reinterpret_cast<const ulonglong2*>(table)[i];  // one 16-byte load
    if (s.x == key) {
      *val_out = (long long)s.y;
      return i;
    }
    if (s.x == kEbEmpty) return -1;
    i = (i + 1) & (cap - 1);
  }
  return -1;
}

// The rehash of both users: every slot of `from` whose value passes `keep_if` claims a slot of `to` (a new, empty table) and stores its value
// there.  Keys of the old table are distinct, so each claims an empty slot and is its only writer.  *kept += slots moved, one integer add per
// wave; a claim that finds no room sets `overflow_bit` in the status word.  Grid-stride; every lane of a wave takes every trip (the ballot).
template <class Keep>
__device__ __forceinline__ void eb_move_slots(const EbSlot* __restrict__ from, long long from_cap, EbSlot* __restrict__ to, long long to_cap, int* status,
                                              int overflow_bit, unsigned long long* kept_out, Keep keep_if) {
  const long long step = (long long)gridDim.x * blockDim.x;
  const long long trips = (from_cap + step - 1) / step;
  for (long long r = 0; r < trips; ++r) {
    const long long i = r * step + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    if (i < from_cap) {
      const ulonglong2 s = reinterpret_cast<const ulonglong2*>(from)[i];
      if (s.x != kEbEmpty && keep_if((long long)s.y)) {
        const long long slot = eb_claim(to, to_cap, s.x);
        if (slot >= 0) {
          to[slot].val = (long long)s.y;
          keep = true;
        } else {
          atomicOr(status, overflow_bit);
        }
      }
    }
    const unsigned long long kept = __ballot(keep);
    if (lane_id() == 0 && kept) atomicAdd(kept_out, (unsigned long long)__popcll(kept));
  }
}

static inline unsigned eb_grid(long long items) {
  const long long blocks = (items + kEbThreads - 1) / kEbThreads;
  return (unsigned)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks));
}

}  // namespace tgmx
