// TGBNegativeEdgeSamplerHook, TGBTHGNegativeEdgeSamplerHook, TGBTKGNegativeEdgeSamplerHook (the reference's tgm/hooks/negatives/tgb_sampler.py)
// for gfx950.  The reference answers a batch of B positives with Q negatives each by B dictionary lookups, B Q int() conversions, B
// host-to-device copies, a cat, a unique (which syncs) and two .item() calls.  The evaluation set is constant for a split, so here it is a
// table on the device, built once, and a batch is
//
//   launch 1   probe + copy + mark: one wave (or, for long rows, one workgroup) per positive finds its row, copies it into the padded
//              matrix with 16-byte loads and stores, and marks every id in a bitmap over [0, max id]
//   launch 2   an ordered compaction of the bitmap = the sorted unique ids; it clears what it read; its tail writes the call's statistics
//              (bitmaps beyond one workgroup's reach: count / scan / write, the scan carrying the tail)
//
// and ONE read of the statistics by the host (the size of the unique set decides a shape: that read is inherent).
//
// The table.  Open addressing, linear probing, capacity a power of two; a slot is 4 bytes, the index of the row that claimed it (-1 empty),
// as analytics.hip's distinct counter: a probe that meets a taken slot compares the 32-byte key of THAT row, read from the keys array no
// launch writes.  Keys of a dictionary are distinct, nothing is ever removed, and after the build the table is read-only: a probe that
// meets an empty slot has seen every slot its key could be in.  Every probe loop is a for over at most `capacity` probes.
//
// The bitmap.  A bit is set by a 32-bit atomicOr, after a plain load has shown it clear (the same few popular destinations are in most
// rows: they would serialise on the atomic unit otherwise).  A stale load costs one atomicOr that changes nothing.  Which lane sets a bit
// does not matter: the result is the same bits from run to run.  The compaction reads every word once, emits its set bits in ascending
// order behind an exclusive scan of the popcounts, and stores 0 where it read anything else, so the next call finds the bitmap clean --
// also after a call that met a missing key.
//
// Everything the launches of one call hand to each other crosses a launch boundary; inside a launch threads meet only in atomics and, in
// the compaction, in LDS behind __syncthreads.
#include "pairtable.h"

namespace tgmx {

constexpr int kTnThreads = 256;
constexpr int kTnWaveRowMax = 1024;          // qpad up to here: one wave per positive, at most 4 trips of 64 lanes x 16 bytes
constexpr int kTnCompactThreads = 1024;      // the one-workgroup compaction: 16 waves
constexpr long long kTnOneWgWords = 16384;   // ... takes bitmaps up to 16 trips (524 288 ids); beyond, the split
constexpr int kTnWordsPerThread = 16;        // the split: a thread owns 16 consecutive words (64 bytes),
constexpr int kTnChunkWords = kTnThreads * kTnWordsPerThread;  // a workgroup 4096
constexpr int kTnNoneMissing = 0x7FFFFFFF;

struct TnKey {
  long long f[4];
};
__device__ __forceinline__ bool operator==(const TnKey& x, const TnKey& y) {
  return x.f[0] == y.f[0] && x.f[1] == y.f[1] && x.f[2] == y.f[2] && x.f[3] == y.f[3];
}
// pairtable.h's splitmix64 finaliser folded over the fields
__device__ __forceinline__ unsigned long long tn_hash(const TnKey& k) {
  unsigned long long h = eb_hash((unsigned long long)k.f[0]);
  h = eb_hash(h ^ (unsigned long long)k.f[1] ^ 0x9E3779B97F4A7C15ull);
  h = eb_hash(h ^ (unsigned long long)k.f[2] ^ 0xD1B54A32D192ED03ull);
  return eb_hash(h ^ (unsigned long long)k.f[3] ^ 0x8CB92BA72F3D8DD7ull);
}
__device__ __forceinline__ TnKey tn_row_key(const int64_t* __restrict__ keys, long long row) {
  const longlong2 a = reinterpret_cast<const longlong2*>(keys)[2 * row], b = reinterpret_cast<const longlong2*>(keys)[2 * row + 1];
  return TnKey{{a.x, a.y, b.x, b.y}};
}

// ---- the build ------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kTnThreads) void tn_insert_kernel(tgmx_tgbneg_t t, int* status) {
  const long long step = (long long)gridDim.x * blockDim.x, mask = t.capacity - 1;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < t.P; p += step) {
    const TnKey key = tn_row_key(t.keys, p);
    long long i = (long long)(tn_hash(key) & (unsigned long long)mask);
    int bits = TGMX_TGBNEG_FULL;
    for (long long probe = 0; probe < t.capacity; ++probe) {
      int cur = __hip_atomic_load(&t.slots[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == -1) {
        cur = atomicCAS(&t.slots[i], -1, (int)p);
        if (cur == -1) {
          bits = 0;
          break;
        }
      }
      if (cur >= 0 && cur < t.P && tn_row_key(t.keys, cur) == key) {
        bits = TGMX_TGBNEG_DUPLICATE;
        break;
      }
      i = (i + 1) & mask;
    }
    if (bits) atomicOr(status, bits);
  }
}

// ---- launch 1 -------------------------------------------------------------------------------------------------------------------------

struct TnBatch {
  const void* v[4];  // src, dst, time, edge type
  int is64[4];
  long long B;
};
__device__ __forceinline__ long long tn_field(const TnBatch& q, int which, long long b) {
  switch (which) {
    case 0: return ld_idx(q.v[0], q.is64[0], b);
    case 1: return ld_idx(q.v[1], q.is64[1], b);
    case 2: return ld_idx(q.v[2], q.is64[2], b);
    case 3: return ld_idx(q.v[3], q.is64[3], b);
    default: return 0;
  }
}
// row of `key`, or -1; the same for every lane that asks with the same key
__device__ __forceinline__ long long tn_find(const tgmx_tgbneg_t& t, const TnKey& key) {
  const long long mask = t.capacity - 1;
  long long i = (long long)(tn_hash(key) & (unsigned long long)mask);
  for (long long probe = 0; probe < t.capacity; ++probe) {
    const int cur = t.slots[i];
    if (cur < 0 || cur >= t.P) return -1;  // empty (or not a row: never written by the build)
    if (tn_row_key(t.keys, cur) == key) return cur;
    i = (i + 1) & mask;
  }
  return -1;
}
__device__ __forceinline__ void tn_mark(unsigned* __restrict__ bitmap, long long words, int id) {
  if (id < 0) return;
  const long long w = id >> 5;
  if (w >= words) return;
  const unsigned bit = 1u << (id & 31);
  if (!(__hip_atomic_load(&bitmap[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(&bitmap[w], bit);
}
__device__ __forceinline__ void tn_mark4(unsigned* __restrict__ bitmap, long long words, const int4& v) {
  tn_mark(bitmap, words, v.x);
  tn_mark(bitmap, words, v.y);
  tn_mark(bitmap, words, v.z);
  tn_mark(bitmap, words, v.w);
}

// per_wave: a workgroup's four waves take four positives, else the whole workgroup takes one.  Either way the unit's lanes all run the same
// probe (uniform loads, no LDS, no barrier) and then stride over the row's 16-byte vectors.
__global__ __launch_bounds__(kTnThreads) void tn_probe_copy_kernel(tgmx_tgbneg_t t, TnBatch q, int per_wave, int32_t* __restrict__ matrix,
                                                                  int32_t* __restrict__ lengths) {
  const int lanes = per_wave ? kWave : kTnThreads, lane = per_wave ? lane_id() : (int)threadIdx.x;
  const int units = per_wave ? kTnThreads / kWave : 1;
  const long long step = (long long)gridDim.x * units;
  const int vecs = t.qpad >> 2;
  for (long long b = (long long)blockIdx.x * units + (per_wave ? threadIdx.x / kWave : 0); b < q.B; b += step) {
    TnKey key;
#pragma unroll
    for (int j = 0; j < 4; ++j) key.f[j] = tn_field(q, t.field[j], b);
    const long long row = tn_find(t, key);
    long long start = 0;
    int len = 0;
    if (row >= 0) {
      start = t.indptr[row];
      len = t.rowlen[row];
      // a row the host laid out wrongly is an empty row, not a read outside the pool
      if (len < 0 || len > t.qpad || start < 0 || (start & 3) || start + ((len + 3) & ~3) > t.pool_ints) len = 0;
    } else if (lane == 0) {
      atomicMin(t.first_missing, (int)b);
    }
    if (lane == 0) lengths[b] = len;
    const int row_vecs = (len + 3) >> 2;
    const int4* __restrict__ in = reinterpret_cast<const int4*>(t.pool + start);
    int4* __restrict__ out = reinterpret_cast<int4*>(matrix + b * t.qpad);
    for (int j = lane; j < vecs; j += lanes) {
      int4 v = make_int4(-1, -1, -1, -1);
      if (j < row_vecs) v = in[j];  // the gap behind a row holds -1
      out[j] = v;
      tn_mark4(t.bitmap, t.bitmap_words, v);
    }
  }
}

// the delegating path's launch 1: the caller filled the matrix
__global__ __launch_bounds__(kTnThreads) void tn_mark_kernel(unsigned* __restrict__ bitmap, long long words, const int32_t* __restrict__ matrix, long long vecs) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < vecs; j += step) tn_mark4(bitmap, words, reinterpret_cast<const int4*>(matrix)[j]);
}

// ---- launch 2: the compaction -----------------------------------------------------------------------------------------------------------

struct TnTail {
  const void* time;
  int time64;
  long long B;
  int* first_missing;
  int64_t* stats;
};

// the set bits of word `word`, ascending, from out[o] on
__device__ __forceinline__ void tn_emit(unsigned w, long long word, long long o, int32_t* __restrict__ out, long long out_cap) {
  while (w) {
    const int bit = __ffs((int)w) - 1;
    w &= w - 1;
    if (o < out_cap) out[o] = (int)(word * 32 + bit);
    ++o;
  }
}
// inclusive scan of one value per thread over the workgroup (blockDim.x a multiple of 64, <= 1024); *total: the workgroup's sum.  Two
// barriers; wave_tot [16] is free again behind the second.
__device__ __forceinline__ long long tn_block_scan(long long v, long long* wave_tot, long long* total) {
  const int lane = lane_id(), wave = threadIdx.x / kWave, waves = blockDim.x / kWave;
  long long incl = v;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const long long o = __shfl_up(incl, off);
    if (lane >= off) incl += o;
  }
  if (lane == kWave - 1) wave_tot[wave] = incl;
  __syncthreads();
  long long before = 0, all = 0;
  for (int w = 0; w < waves; ++w) {
    const long long x = wave_tot[w];
    if (w < wave) before += x;
    all += x;
  }
  __syncthreads();
  *total = all;
  return before + incl;
}
// by ONE workgroup: {n, min(time), max(time), first missing or -1} into stats, first_missing armed for the next call
__device__ __forceinline__ void tn_write_stats(const TnTail& a, long long n, long long* red) {  // red: 2 x 16 in LDS
  long long lo = 0x7FFFFFFFFFFFFFFFll, hi = -0x7FFFFFFFFFFFFFFFll - 1;
  for (long long i = threadIdx.x; i < a.B; i += blockDim.x) {
    const long long v = ld_idx(a.time, a.time64, i);
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const long long l2 = __shfl_xor(lo, off), h2 = __shfl_xor(hi, off);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  const int wave = threadIdx.x / kWave, waves = blockDim.x / kWave;
  if (lane_id() == 0) red[wave] = lo, red[16 + wave] = hi;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < waves; ++w) {
      lo = red[w] < lo ? red[w] : lo;
      hi = red[16 + w] > hi ? red[16 + w] : hi;
    }
    const int miss = *a.first_missing;
    a.stats[0] = n;
    a.stats[1] = lo;
    a.stats[2] = hi;
    a.stats[3] = miss == kTnNoneMissing ? -1 : miss;
    *a.first_missing = kTnNoneMissing;
  }
}

// ONE workgroup strides over chunks of blockDim.x words; the base is carried from chunk to chunk: the output order is the id order
__global__ __launch_bounds__(kTnCompactThreads) void tn_compact_one_kernel(unsigned* __restrict__ bitmap, long long words, int32_t* __restrict__ out,
                                                                          long long out_cap, TnTail tail) {
  __shared__ long long wave_tot[32];
  long long carry = 0;  // the same in every thread
  for (long long r0 = 0; r0 < words; r0 += blockDim.x) {
    const long long i = r0 + threadIdx.x;
    const unsigned w = i < words ? bitmap[i] : 0u;
    const int c = __popc(w);
    long long total;
    const long long incl = tn_block_scan(c, wave_tot, &total);
    if (w) {
      tn_emit(w, i, carry + incl - c, out, out_cap);
      bitmap[i] = 0u;
    }
    carry += total;
  }
  tn_write_stats(tail, carry < out_cap ? carry : out_cap, wave_tot);
}

// the split, for bitmaps of a multiple of kTnChunkWords words: (1) set bits per workgroup of kTnChunkWords words
__global__ __launch_bounds__(kTnThreads) void tn_count_kernel(const unsigned* __restrict__ bitmap, int32_t* __restrict__ block_counts) {
  __shared__ long long wave_tot[16];
  const uint4* __restrict__ p = reinterpret_cast<const uint4*>(bitmap + ((long long)blockIdx.x * kTnThreads + threadIdx.x) * kTnWordsPerThread);
  int c = 0;
#pragma unroll
  for (int k = 0; k < kTnWordsPerThread / 4; ++k) {
    const uint4 v = p[k];
    c += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
  }
  long long total;
  tn_block_scan(c, wave_tot, &total);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = (int)total;
}
// (2) ONE workgroup: block_counts -> their exclusive scan, in place; then the statistics
__global__ __launch_bounds__(kTnCompactThreads) void tn_scan_kernel(int32_t* __restrict__ block_counts, long long blocks, long long out_cap, TnTail tail) {
  __shared__ long long wave_tot[32];
  long long carry = 0;
  for (long long r0 = 0; r0 < blocks; r0 += blockDim.x) {
    const long long i = r0 + threadIdx.x;
    const int c = i < blocks ? block_counts[i] : 0;
    long long total;
    const long long incl = tn_block_scan(c, wave_tot, &total);
    if (i < blocks) block_counts[i] = (int)(carry + incl - c);  // < 2^31: there are no more ids than that
    carry += total;
  }
  tn_write_stats(tail, carry < out_cap ? carry : out_cap, wave_tot);
}
// (3) every workgroup emits its words behind its base and clears them
__global__ __launch_bounds__(kTnThreads) void tn_write_kernel(unsigned* __restrict__ bitmap, const int32_t* __restrict__ block_base, int32_t* __restrict__ out,
                                                             long long out_cap) {
  __shared__ long long wave_tot[16];
  const long long word0 = ((long long)blockIdx.x * kTnThreads + threadIdx.x) * kTnWordsPerThread;
  uint4* __restrict__ p = reinterpret_cast<uint4*>(bitmap + word0);
  uint4 v[kTnWordsPerThread / 4];
  int c = 0;
#pragma unroll
  for (int k = 0; k < kTnWordsPerThread / 4; ++k) {
    v[k] = p[k];
    c += __popc(v[k].x) + __popc(v[k].y) + __popc(v[k].z) + __popc(v[k].w);
  }
  long long total;
  const long long incl = tn_block_scan(c, wave_tot, &total);
  if (c == 0) return;  // behind the scan's barriers
  long long o = (long long)block_base[blockIdx.x] + incl - c;
#pragma unroll
  for (int k = 0; k < kTnWordsPerThread / 4; ++k) {
    const unsigned w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      tn_emit(w[e], word0 + 4 * k + e, o, out, out_cap);
      o += __popc(w[e]);
    }
    p[k] = make_uint4(0u, 0u, 0u, 0u);
  }
}

static bool tn_pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }

static int tn_check_scratch(const tgmx_tgbneg_t& t, const char* what) {
  TGMX_REQUIRE(t.bitmap && t.first_missing && t.bitmap_words > 0 && t.bitmap_words <= (1ll << 26), "%s: no bitmap, or one of %lld words", what,
               (long long)t.bitmap_words);
  TGMX_REQUIRE(t.qpad > 0 && (t.qpad & 3) == 0, "%s: qpad %d is no positive multiple of four", what, (int)t.qpad);
  if (t.bitmap_words > kTnOneWgWords) {
    TGMX_REQUIRE(t.bitmap_words % kTnChunkWords == 0, "%s: a bitmap of %lld words must be a multiple of %d", what, (long long)t.bitmap_words, kTnChunkWords);
    TGMX_REQUIRE(t.block_counts && t.num_blocks >= t.bitmap_words / kTnChunkWords, "%s: block_counts holds %lld of %lld entries", what,
                 (long long)t.num_blocks, (long long)(t.bitmap_words / kTnChunkWords));
  }
  return TGMX_OK;
}

static int tn_compact(const tgmx_tgbneg_t& t, int32_t* neg, long long neg_cap, const TnTail& tail, hipStream_t st) {
  unsigned* bitmap = reinterpret_cast<unsigned*>(t.bitmap);
  if (t.bitmap_words <= kTnOneWgWords) {
    hipLaunchKernelGGL(tn_compact_one_kernel, dim3(1), dim3(kTnCompactThreads), 0, st, bitmap, (long long)t.bitmap_words, neg, neg_cap, tail);
    TGMX_CHECK_LAUNCH("tgbneg(compact)");
    return TGMX_OK;
  }
  const long long blocks = t.bitmap_words / kTnChunkWords;
  hipLaunchKernelGGL(tn_count_kernel, dim3((unsigned)blocks), dim3(kTnThreads), 0, st, (const unsigned*)bitmap, t.block_counts);
  TGMX_CHECK_LAUNCH("tgbneg(count)");
  hipLaunchKernelGGL(tn_scan_kernel, dim3(1), dim3(kTnCompactThreads), 0, st, t.block_counts, blocks, neg_cap, tail);
  TGMX_CHECK_LAUNCH("tgbneg(scan)");
  hipLaunchKernelGGL(tn_write_kernel, dim3((unsigned)blocks), dim3(kTnThreads), 0, st, bitmap, (const int32_t*)t.block_counts, neg, neg_cap);
  TGMX_CHECK_LAUNCH("tgbneg(write)");
  return TGMX_OK;
}

}  // namespace tgmx

using namespace tgmx;

extern "C" int64_t tgmx_tgbneg_limit(int32_t which) {
  switch (which) {
    case 0: return kTnWaveRowMax;
    case 1: return kTnOneWgWords;
    case 2: return kTnChunkWords;
    default: return -1;
  }
}

extern "C" int tgmx_tgbneg_build(const tgmx_tgbneg_t* t, int32_t* status, tgmx_stream_t stream) {
  TGMX_REQUIRE(t && status && t->keys && t->slots, "tgbneg_build: null pointer");
  TGMX_REQUIRE(t->P > 0 && t->P < (1ll << 31) && tn_pow2(t->capacity) && t->capacity > t->P, "tgbneg_build: %lld rows in %lld slots (a power of two above the rows)",
               (long long)t->P, (long long)t->capacity);
  hipLaunchKernelGGL(tn_insert_kernel, dim3(eb_grid(t->P)), dim3(kTnThreads), 0, (hipStream_t)stream, *t, status);
  TGMX_CHECK_LAUNCH("tgbneg_build");
  return TGMX_OK;
}

extern "C" int tgmx_tgbneg_query(const tgmx_tgbneg_t* t, const void* src, int32_t src_is64, const void* dst, int32_t dst_is64, const void* time,
                                 int32_t time_is64, const void* etype, int32_t etype_is64, int64_t B, int32_t* matrix, int32_t* neg, int64_t neg_cap,
                                 int64_t* stats, tgmx_stream_t stream) {
  TGMX_REQUIRE(t && t->keys && t->indptr && t->rowlen && t->pool && t->slots, "tgbneg_query: null table pointer");
  TGMX_REQUIRE(t->P > 0 && t->P < (1ll << 31) && tn_pow2(t->capacity) && t->capacity > t->P && t->pool_ints >= 0, "tgbneg_query: bad table sizes");
  if (int rc = tn_check_scratch(*t, "tgbneg_query")) return rc;
  TGMX_REQUIRE(B > 0 && B < (1ll << 31) && matrix && neg && stats && time && neg_cap >= 0, "tgbneg_query: B = %lld, or a null pointer", (long long)B);
  TnBatch q{{src, dst, time, etype}, {src_is64 != 0, dst_is64 != 0, time_is64 != 0, etype_is64 != 0}, (long long)B};
  for (int j = 0; j < 4; ++j) {
    const int f = t->field[j];
    TGMX_REQUIRE(f >= -1 && f < 4 && (f < 0 || q.v[f]), "tgbneg_query: key column %d names batch field %d, which is out of range or has no pointer", j, f);
  }
  hipStream_t st = (hipStream_t)stream;
  const int per_wave = t->qpad <= kTnWaveRowMax;
  const long long units = per_wave ? kTnThreads / kWave : 1, blocks = (B + units - 1) / units;
  hipLaunchKernelGGL(tn_probe_copy_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(kTnThreads), 0, st, *t, q, per_wave, matrix,
                     reinterpret_cast<int32_t*>(stats + 4));
  TGMX_CHECK_LAUNCH("tgbneg_query(probe)");
  return tn_compact(*t, neg, (long long)neg_cap, TnTail{time, time_is64 != 0, (long long)B, t->first_missing, stats}, st);
}

extern "C" int tgmx_tgbneg_unique(const tgmx_tgbneg_t* t, const int32_t* matrix, int64_t B, const void* time, int32_t time_is64, int32_t* neg,
                                  int64_t neg_cap, int64_t* stats, tgmx_stream_t stream) {
  TGMX_REQUIRE(t, "tgbneg_unique: null pointer");
  if (int rc = tn_check_scratch(*t, "tgbneg_unique")) return rc;
  TGMX_REQUIRE(B > 0 && B < (1ll << 31) && matrix && neg && stats && time && neg_cap >= 0, "tgbneg_unique: B = %lld, or a null pointer", (long long)B);
  hipStream_t st = (hipStream_t)stream;
  const long long vecs = (long long)B * (t->qpad >> 2);
  hipLaunchKernelGGL(tn_mark_kernel, dim3(eb_grid(vecs)), dim3(kTnThreads), 0, st, reinterpret_cast<unsigned*>(t->bitmap), (long long)t->bitmap_words, matrix, vecs);
  TGMX_CHECK_LAUNCH("tgbneg_unique(mark)");
  return tn_compact(*t, neg, (long long)neg_cap, TnTail{time, time_is64 != 0, (long long)B, t->first_missing, stats}, st);
}
