// DensityOfStateEstimatorHook past the LDS route's 4096 events (dos.hip), for gfx950: the same estimate over a snapshot-sized graph
// (4096 < E <= 2^22 events: a day or a week of a stream), its operator a CSR in HBM.  One call, nothing read back; every grid is sized from
// 2 E, the node and entry counts stay in device header words.
//
//   1. the CSR of S = L_norm - I.  2 E directed keys (row id << 31 | col id: edge_csr.h's keys at 31 column bits; an event with an endpoint
//      outside [0, 2^31) gets the key behind every row and flags *status), ONE rocPRIM radix sort over 63 bits.  Equal neighbours are dropped
//      by a three-launch scan (a workgroup counts the entries and row heads of its 8192 sorted keys; one workgroup scans the <= 1024 counts;
//      the workgroups scan again and scatter): row heads -> node ids and indptr, entries -> column ids.  A launch over the entries then finds
//      every column's local index by binary search of the node ids and stores -1 / sqrt(d_i d_j), evaluated as the LDS route evaluates it;
//      the same launch counts, and a second scan lists, the rows longer than kDosChunk as chunks of that many entries -- the LDS route's
//      scheme without a ceiling: the lists live in the workspace, one row may hold every entry.
//   2. the moments, ONE launch without any grid-wide synchronisation.  Probe columns are independent: a workgroup owns a slab of PV columns
//      for all n rows and all nM moments and loops over slabs where there are more slabs than workgroups.  Lanes run along the PV columns of
//      a row.  T_m overwrites T_{m-2} in place (element (i, p) of T_{m-2} is read by its owner only), the two block pointers swap: one
//      workgroup barrier per moment, a second while chunk partials are combined.  The two [n, PV] blocks are LDS when n <= lds_rows, else
//      the workgroup's own region of the workspace -- decided on the device from the header's n, uniformly over the workgroup, as two
//      instantiations of one body over LDS-typed and global-typed pointers.  CSR entries stream from global memory (the same for every slab,
//      cache-resident at snapshot sizes).  Z is never stored: a sign is one counter_u32 call.
//   3. dos_finish_kernel (dos_shared.h), unchanged.
//
// Determinism as in dos.hip: no float atomics; a row's sum runs over its entries in CSR order, a chunked row's partial sums are added chunk
// by chunk by the row's owner, a moment's column sum goes thread (rows ascending) -> wave (xor tree) -> workgroup (waves ascending) in
// double.  The order is fixed by the CSR and by (E, nZ) through the launch geometry, never by timing: equal inputs give equal bits.
//
// Matrix instructions do not fit: a row holds a handful of entries, there is no dense tile to feed an MFMA with.
#include <algorithm>

#include "dos_shared.h"
#include "edge_csr.h"

namespace tgmx {

constexpr long long kDlMinE = 4097, kDlMaxE = 1ll << 22;
constexpr int kDlCb = 31;                 // column bits of a key
constexpr int kDlThreads = 1024;          // scan kernels and the moments kernel: 16 waves
constexpr int kDlWaves = kDlThreads / kWave;
constexpr int kDlPer = 8;                 // consecutive keys (rows) a scan thread owns
constexpr int kDlTile = kDlThreads * kDlPer;  // 8192 a workgroup: 2 E <= 2^23 keys are <= 1024 tiles, which ONE workgroup scans
constexpr int kDlFill = 32;               // the PV rule: slabs wanted before a slab gets wider
constexpr int kDlMaxGroups = 256;         // moments workgroups at most: one a CU
constexpr size_t kDlTBudget = 1ull << 30; // bytes of T regions at most (one region at least)
// dynamic LDS of the moments kernel: the 160 KB less 4 KB for its static LDS (the waves' column sums)
constexpr size_t kDlLdsBytes = kDosLdsBudget - 4096;

enum { kDlN = 0, kDlNnz = 1, kDlNChunks = 2, kDlNSplit = 3 };  // header words

typedef unsigned long long u64;
typedef __attribute__((address_space(3))) float* LdsFloats;
typedef __attribute__((address_space(1))) float* GlobalFloats;

struct DosLargeArgs {
  const void* src;
  const void* dst;
  int E, src64, dst64;
  int nmax;       // 2 E: keys, and the most rows and entries
  int nZ, nM, n_pts, PV;
  int nslabs, lds_rows, max_chunks, max_split;
  u64 seed, call;
  int* head;      // [64]
  u64* keys;      // [2 E] sorted
  int* erow;      // [2 E]: an entry's row (in the bytes of the unsorted keys)
  int* node_id;   // [2 E]
  int* indptr;    // [2 E + 1]
  int* cols;      // [2 E]
  float* vals;    // [2 E]
  u64* blk_cnt;   // [1024]
  u64* blk_base;  // [1024]
  int* chunks;    // [max_chunks][2]: begin, end
  int* split;     // [max_split][3]: row, first chunk, chunks
  float* tws;     // [groups][t_stride]: T_{m-1}, T_{m-2} [2 E, PV] each, then the chunks' partial sums [max_chunks, PV]
  size_t t_stride;
  double* cmom;   // [nM, nZ]
  double* cdf;    // [n_pts]
  double* dos;    // [n_pts - 1]
  u64* status;
};

// ---- 1. the graph as the CSR of S ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void dos_large_keys_kernel(DosLargeArgs a) {
  bool bad = false;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < a.E; e += gridDim.x * blockDim.x) {
    const long long s = ld_idx(a.src, a.src64, e), d = ld_idx(a.dst, a.dst64, e);
    const bool keep = s >= 0 && d >= 0 && s < (1ll << 31) && d < (1ll << 31);
    bad |= !keep;
    a.keys[2 * e] = key_of(keep, s, d, kDlCb);  // (unsorted: the launch gets the sort's input for `keys`)
    a.keys[2 * e + 1] = key_of(keep, d, s, kDlCb);
  }
  if (bad) atomicOr(a.status, (u64)TGMX_AN_BAD_ID);
}

// the thread's kDlPer consecutive sorted keys: which are the first of their value (an entry), which the first of their row (a head);
// returns entries << 32 | heads
__device__ __forceinline__ u64 dos_large_flags(const DosLargeArgs& a, u64* mine, unsigned* is_entry, unsigned* is_head) {
  const int first = blockIdx.x * kDlTile + threadIdx.x * kDlPer;
  u64 cnt = 0, prev = first > 0 && first <= a.nmax ? a.keys[first - 1] : 0;
  *is_entry = *is_head = 0;
#pragma unroll
  for (int q = 0; q < kDlPer; ++q) {
    const int idx = first + q;
    const u64 key = idx < a.nmax ? a.keys[idx] : key_behind(kDlCb);
    mine[q] = key;
    if (key < key_behind(kDlCb)) {
      const bool entry = idx == 0 || key != prev, head = idx == 0 || key_row(key, kDlCb) != key_row(prev, kDlCb);
      *is_entry |= (unsigned)entry << q;
      *is_head |= (unsigned)head << q;
      cnt += ((u64)entry << 32) + (u64)head;
    }
    prev = key;
  }
  return cnt;
}

__global__ __launch_bounds__(kDlThreads) void dos_large_count_kernel(DosLargeArgs a) {
  __shared__ u64 s_wave[kDlWaves];
  u64 mine[kDlPer], total;
  unsigned is_entry, is_head;
  dos_block_scan(dos_large_flags(a, mine, &is_entry, &is_head), s_wave, &total);
  if (threadIdx.x == 0) a.blk_cnt[blockIdx.x] = total;
}

// ONE workgroup: the exclusive scan of the tiles' packed counts; the totals go to two header words (hi, lo).  indptr != NULL: the counts
// are (entries, heads), and the row pointer behind the last row is the entry count.
__global__ __launch_bounds__(kDlThreads) void dos_large_scan_kernel(const u64* __restrict__ cnt, u64* __restrict__ base, int tiles, int* head,
                                                                    int word_hi, int word_lo, int* indptr) {
  __shared__ u64 s_wave[kDlWaves];
  const int tid = threadIdx.x;
  u64 total;
  const u64 before = dos_block_scan(tid < tiles ? cnt[tid] : 0ull, s_wave, &total);
  if (tid < tiles) base[tid] = before;
  if (tid == 0) {
    head[word_hi] = (int)(total >> 32);
    head[word_lo] = (int)(total & 0xFFFFFFFFull);
    if (indptr) indptr[(int)(total & 0xFFFFFFFFull)] = (int)(total >> 32);
  }
}

__global__ __launch_bounds__(kDlThreads) void dos_large_scatter_kernel(DosLargeArgs a) {
  __shared__ u64 s_wave[kDlWaves];
  u64 mine[kDlPer], total;
  unsigned is_entry, is_head;
  const u64 cnt = dos_large_flags(a, mine, &is_entry, &is_head);
  const u64 base = a.blk_base[blockIdx.x] + dos_block_scan(cnt, s_wave, &total);
  int pos = (int)(base >> 32), row = (int)(base & 0xFFFFFFFFull) - 1;  // row of the key before this thread's first
#pragma unroll
  for (int q = 0; q < kDlPer; ++q) {
    if ((is_head >> q) & 1u) {  // a head is an entry: pos < nmax and row < nmax, the key counts bound both
      ++row;
      a.node_id[row] = (int)key_row(mine[q], kDlCb);
      a.indptr[row] = pos;
    }
    if ((is_entry >> q) & 1u) {
      a.cols[pos] = (int)key_col(mine[q], kDlCb);  // the global id: dos_large_entries_kernel makes it the local index
      a.erow[pos] = row;
      ++pos;
    }
  }
}

// rows kDlPer in a row a thread: (rows longer than a chunk) << 32 | their chunks
__device__ __forceinline__ u64 dos_large_long_rows(const DosLargeArgs& a, int n) {
  const int first = blockIdx.x * kDlTile + threadIdx.x * kDlPer;
  u64 cnt = 0;
  for (int r = first; r < min(n, first + kDlPer); ++r) {
    const int len = a.indptr[r + 1] - a.indptr[r];
    if (len > kDosChunk) cnt += (1ull << 32) + (u64)((len + kDosChunk - 1) / kDosChunk);
  }
  return cnt;
}

// every entry: its column's local index (every column id is a row id: the key set is symmetric) and its value, -1 / sqrt(d_i d_j) as ONE
// float expression: the degrees converted to float (exact, <= 2^23), their float product (rounded once where it needs more than 24 bits),
// IEEE sqrt, IEEE divide of -1 by it.  The product commutes: S_ij == S_ji.  Then the tile's count of long rows.
__global__ __launch_bounds__(kDlThreads) void dos_large_entries_kernel(DosLargeArgs a) {
  __shared__ u64 s_wave[kDlWaves];
  const int n = a.head[kDlN], nnz = a.head[kDlNnz];
  for (int q = 0; q < kDlPer; ++q) {
    const int t = blockIdx.x * kDlTile + q * kDlThreads + threadIdx.x;
    if (t >= nnz) break;
    const int row = a.erow[t], cid = a.cols[t];
    int lo = 0, hi = n;  // lower bound of cid in node_id [0, n)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.node_id[mid] < cid) lo = mid + 1;
      else hi = mid;
    }
    const int j = lo < n ? lo : n - 1;
    const float di = (float)(a.indptr[row + 1] - a.indptr[row]), dj = (float)(a.indptr[j + 1] - a.indptr[j]);
    a.cols[t] = j;
    a.vals[t] = -1.f / __fsqrt_rn(di * dj);
  }
  u64 total;
  dos_block_scan(dos_large_long_rows(a, n), s_wave, &total);
  if (threadIdx.x == 0) a.blk_cnt[blockIdx.x] = total;
}

// the work list of long rows: a thread owns consecutive rows and the tiles are scanned in order, so the list is in row order
__global__ __launch_bounds__(kDlThreads) void dos_large_chunks_kernel(DosLargeArgs a) {
  __shared__ u64 s_wave[kDlWaves];
  const int n = a.head[kDlN];
  u64 total;
  const u64 base = a.blk_base[blockIdx.x] + dos_block_scan(dos_large_long_rows(a, n), s_wave, &total);
  int sp = (int)(base >> 32), ch = (int)(base & 0xFFFFFFFFull);
  const int first = blockIdx.x * kDlTile + threadIdx.x * kDlPer;
  for (int r = first; r < min(n, first + kDlPer); ++r) {
    const int b = a.indptr[r], e = a.indptr[r + 1];
    if (e - b <= kDosChunk) continue;
    const int c = (e - b + kDosChunk - 1) / kDosChunk;
    if (sp < a.max_split && ch + c <= a.max_chunks) {  // always (dos_large_plan's bounds); a guard for the stores
      a.split[3 * sp] = r, a.split[3 * sp + 1] = ch, a.split[3 * sp + 2] = c;
      for (int q = 0; q < c; ++q) a.chunks[2 * (ch + q)] = b + q * kDosChunk, a.chunks[2 * (ch + q) + 1] = min(e, b + (q + 1) * kDosChunk);
    }
    ++sp;
    ch += c;
  }
}

// ---- 2. the Chebyshev moments of the slabs of probe columns ---------------------------------------------------------------------------

// TP: the address space of the two T blocks.  Called uniformly by the whole workgroup.
template <int PV, typename TP>
__device__ __forceinline__ void dos_large_slabs(const DosLargeArgs& a, int n, int nchunks, int nsplit, TP cur, TP old, float* part,
                                                double* s_cw) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  constexpr int RP = kDlThreads / PV;  // rows a pass of the workgroup covers
  const int grp = tid / PV, p = tid % PV;
  const int* __restrict__ indptr = a.indptr;
  const int* __restrict__ cols = a.cols;
  const float* __restrict__ vals = a.vals;
  const int* __restrict__ node_id = a.node_id;

  for (int slab = blockIdx.x; slab < a.nslabs; slab += gridDim.x) {
    const int col = slab * PV + p;  // past nZ in the last slab's tail: computed, not stored
    // T_0 = Z, and c_0 = n
    double dsum = 0.0;
    for (int i = grp; i < n; i += RP) {
      cur[i * PV + p] = dos_sign(a.seed, a.call, a.nZ, node_id[i], col);
      dsum += 1.0;
    }
    for (int m = 0; m < a.nM; ++m) {
      if (m > 0) {  // behind the barrier that ended moment m - 1: T_{m-1} is complete
        dsum = 0.0;
        for (int i = grp; i < n; i += RP) {
          const int b = indptr[i], e = indptr[i + 1];
          if (e - b > kDosChunk) continue;  // a chunked row: below
          float acc = 0.f;
          for (int q = b; q < e; ++q) acc = __fmaf_rn(vals[q], cur[cols[q] * PV + p], acc);
          const float t = m == 1 ? acc : __fmaf_rn(2.f, acc, -old[i * PV + p]);
          old[i * PV + p] = t;
          dsum += (double)(t * dos_sign(a.seed, a.call, a.nZ, node_id[i], col));
        }
        if (nsplit > 0) {  // uniform over the workgroup
          for (int c = grp; c < nchunks; c += RP) {
            float acc = 0.f;
            for (int q = a.chunks[2 * c]; q < a.chunks[2 * c + 1]; ++q) acc = __fmaf_rn(vals[q], cur[cols[q] * PV + p], acc);
            part[(size_t)c * PV + p] = acc;
          }
          __syncthreads();  // the workgroup's own stores to part are visible to it
          for (int s = grp; s < nsplit; s += RP) {
            const int i = a.split[3 * s], c0 = a.split[3 * s + 1], cn = a.split[3 * s + 2];
            float acc = 0.f;
            for (int c = c0; c < c0 + cn; ++c) acc += part[(size_t)c * PV + p];  // chunk by chunk, in row order
            const float t = m == 1 ? acc : __fmaf_rn(2.f, acc, -old[i * PV + p]);
            old[i * PV + p] = t;
            dsum += (double)(t * dos_sign(a.seed, a.call, a.nZ, node_id[i], col));
          }
        }
        const TP sw = cur;
        cur = old;
        old = sw;
      }
      // c[m, col] = sum over the rows: the lanes of a wave that share p (xor tree), then the waves in order
#pragma unroll
      for (int off = PV; off < kWave; off <<= 1) dsum += __shfl_xor(dsum, off);
      double* cw = s_cw + (m & 1) * kDlWaves * PV;
      if (lane < PV) cw[wave * PV + lane] = dsum;
      __syncthreads();  // the moment's one barrier (T_m, in LDS or in the workgroup's region, is visible to the workgroup behind it).
                        // Moment m + 2 writes cw again only behind the barrier of m + 1, which wave 0 reaches after its read
      if (tid < PV && col < a.nZ) {
        double c = 0.0;
#pragma unroll
        for (int w = 0; w < kDlWaves; ++w) c += cw[w * PV + tid];
        a.cmom[(size_t)m * a.nZ + col] = c;
      }
    }
    __syncthreads();  // the next slab writes T_0 and cw[0]: every read of this slab is done
  }
}

template <int PV>
__global__ __launch_bounds__(kDlThreads) void dos_large_moments_kernel(DosLargeArgs a) {
  extern __shared__ float dos_large_lds[];  // [2][lds_rows][PV]
  __shared__ double s_cw[2 * kDlWaves * PV];
  const int n = a.head[kDlN], nchunks = min(a.head[kDlNChunks], a.max_chunks), nsplit = min(a.head[kDlNSplit], a.max_split);  // (never more)
  float* region = a.tws + (size_t)blockIdx.x * a.t_stride;
  float* part = region + 2 * (size_t)a.nmax * PV;
  if (n <= a.lds_rows) {
    const LdsFloats t = (LdsFloats)dos_large_lds;
    dos_large_slabs<PV, LdsFloats>(a, n, nchunks, nsplit, t, t + (size_t)a.lds_rows * PV, part, s_cw);
  } else {
    const GlobalFloats t = (GlobalFloats)region;
    dos_large_slabs<PV, GlobalFloats>(a, n, nchunks, nsplit, t, t + (size_t)a.nmax * PV, part, s_cw);
  }
}

// ---- the host's plan: PV, the grid, the workspace ------------------------------------------------------------------------------------------

// The PV rule.  A wider slab reads the CSR fewer times (once a slab a moment) and makes a row's gather of T one 4 PV-byte segment, but a
// workgroup walks all n rows alone, so the slabs are what fills the device: PV is the widest of {8, 4, 2, 1} that still leaves kDlFill slabs,
// 1 where even that leaves fewer.
static int dos_large_width(int nZ) {
  for (int pv = 8; pv > 1; pv >>= 1)
    if ((nZ + pv - 1) / pv >= kDlFill) return pv;
  return 1;
}
static int dos_large_lds_rows(int pv) { return (int)(kDlLdsBytes / (2 * sizeof(float) * pv)); }

struct DosLargePlan {
  int pv, nslabs, groups, tiles, max_chunks, max_split;
  size_t t_stride, temp_bytes, total;
  u64* k_in;   // the sort's input; an entry's row later
  char* temp;  // the sort's own
};
static bool dos_large_in_envelope(long long E, int nZ, int nM, int n_pts) {
  return E >= kDlMinE && E <= kDlMaxE && nZ >= 1 && nZ <= 1024 && nM >= 2 && nM <= 64 && n_pts >= 2 && n_pts <= 65536;
}
// the regions of the workspace, in order (workspace NULL: the sizes only)
static void dos_large_plan(void* workspace, long long E, int nZ, int nM, int n_pts, DosLargePlan& pl, DosLargeArgs* a) {
  const size_t nmax = 2 * (size_t)E;
  pl.pv = dos_large_width(nZ);
  pl.nslabs = (nZ + pl.pv - 1) / pl.pv;
  pl.tiles = (int)((nmax + kDlTile - 1) / kDlTile);
  // rows longer than a chunk hold > kDosChunk entries each, and their chunks number sum ceil(len / kDosChunk) <= nnz / kDosChunk + rows
  pl.max_split = (int)(nmax / (kDosChunk + 1)) + 1;
  pl.max_chunks = (int)(nmax / kDosChunk) + pl.max_split;
  pl.t_stride = ((2 * nmax + (size_t)pl.max_chunks) * pl.pv + 63) & ~(size_t)63;
  const size_t fit = kDlTBudget / (pl.t_stride * sizeof(float));
  pl.groups = (int)std::min<size_t>(std::min<size_t>(pl.nslabs, kDlMaxGroups), std::max<size_t>(fit, 1));
  // The sort's own storage is reserved by a bound, not by rocPRIM's query: the query needs a device, the size of the workspace must not.  The
  // sort keeps a second copy of the keys (8 bytes a key) plus histograms and per-block scan states (under a byte a key as rocPRIM is built
  // here); tgmx_dos_large_estimate makes the query and refuses to run if the bound should ever fall short.
  pl.temp_bytes = 16 * nmax + (1u << 20);
  WorkspaceCarver c(workspace);
  int* head = c.take<int>(64);
  u64* k_in = c.take<u64>(nmax);
  u64* k_out = c.take<u64>(nmax);
  char* temp = c.take<char>(pl.temp_bytes);
  int* node_id = c.take<int>(nmax);
  int* indptr = c.take<int>(nmax + 1);
  int* cols = c.take<int>(nmax);
  float* vals = c.take<float>(nmax);
  u64* blk_cnt = c.take<u64>(kDlThreads);
  u64* blk_base = c.take<u64>(kDlThreads);
  int* chunks = c.take<int>(2 * (size_t)pl.max_chunks);
  int* split = c.take<int>(3 * (size_t)pl.max_split);
  double* cmom = c.take<double>((size_t)nM * nZ);
  double* cdf = c.take<double>((size_t)n_pts);
  float* tws = c.take<float>((size_t)pl.groups * pl.t_stride);
  pl.total = c.total();
  if (a) {
    a->head = head, a->keys = k_out, a->erow = reinterpret_cast<int*>(k_in), a->node_id = node_id, a->indptr = indptr, a->cols = cols, a->vals = vals;
    a->blk_cnt = blk_cnt, a->blk_base = blk_base, a->chunks = chunks, a->split = split, a->cmom = cmom, a->cdf = cdf, a->tws = tws;
    a->t_stride = pl.t_stride, a->max_chunks = pl.max_chunks, a->max_split = pl.max_split;
    a->PV = pl.pv, a->nslabs = pl.nslabs, a->lds_rows = dos_large_lds_rows(pl.pv);
  }
  pl.k_in = k_in, pl.temp = temp;
}

}  // namespace tgmx

using namespace tgmx;

extern "C" int32_t tgmx_dos_large_supported(int64_t E, int32_t nZ, int32_t nM, int32_t n_pts) { return dos_large_in_envelope(E, nZ, nM, n_pts); }

extern "C" int32_t tgmx_dos_large_probe_width(int64_t E, int32_t nZ) {
  return E >= kDlMinE && E <= kDlMaxE && nZ >= 1 && nZ <= 1024 ? dos_large_width(nZ) : 0;
}

extern "C" int32_t tgmx_dos_large_lds_rows(int64_t E, int32_t nZ) {
  const int pv = tgmx_dos_large_probe_width(E, nZ);
  return pv ? dos_large_lds_rows(pv) : 0;
}

extern "C" size_t tgmx_dos_large_workspace_bytes(int64_t E, int32_t nZ, int32_t nM, int32_t n_pts) {
  DosLargePlan pl;
  if (!dos_large_in_envelope(E, nZ, nM, n_pts)) return 0;
  dos_large_plan(nullptr, E, nZ, nM, n_pts, pl, nullptr);
  return pl.total;
}

extern "C" int tgmx_dos_large_estimate(const tgmx_dos_large_t* args, tgmx_stream_t stream) {
  TGMX_REQUIRE(args, "dos_large_estimate: null pointer");
  const tgmx_dos_large_t& t = *args;
  TGMX_REQUIRE(dos_large_in_envelope(t.E, t.nZ, t.nM, t.n_pts), "dos_large_estimate: outside the envelope (E=%lld nZ=%d nM=%d n_pts=%d)", (long long)t.E,
               t.nZ, t.nM, t.n_pts);
  TGMX_REQUIRE(t.src && t.dst && t.dos && t.status && t.workspace, "dos_large_estimate: null pointer");
  DosLargeArgs a{};
  DosLargePlan pl;
  dos_large_plan(t.workspace, t.E, t.nZ, t.nM, t.n_pts, pl, &a);
  size_t sort_bytes = 0;
  if (rocprim::radix_sort_keys(nullptr, sort_bytes, (const u64*)nullptr, (u64*)nullptr, 2 * (size_t)t.E, 0u, (unsigned)(2 * kDlCb + 1)) != hipSuccess) {
    set_error("dos_large_estimate: the sort's storage query failed");
    return TGMX_E_LAUNCH;
  }
  TGMX_REQUIRE(sort_bytes <= pl.temp_bytes, "dos_large_estimate: the sort asks for %zu bytes, %zu are reserved", sort_bytes, pl.temp_bytes);
  TGMX_REQUIRE(t.workspace_bytes >= pl.total, "dos_large_estimate: workspace too small (%zu of %zu bytes)", t.workspace_bytes, pl.total);
  a.src = t.src, a.dst = t.dst, a.E = (int)t.E, a.src64 = t.src_is64 != 0, a.dst64 = t.dst_is64 != 0, a.nmax = (int)(2 * t.E);
  a.nZ = t.nZ, a.nM = t.nM, a.n_pts = t.n_pts, a.seed = t.seed, a.call = t.call;
  a.dos = t.dos, a.status = reinterpret_cast<u64*>(t.status);
  hipStream_t st = (hipStream_t)stream;
  const dim3 tiles((unsigned)pl.tiles), wg(kDlThreads);

  {  // the keys kernel writes the sort's input
    DosLargeArgs k = a;
    k.keys = pl.k_in;
    hipLaunchKernelGGL(dos_large_keys_kernel, dim3(grid_for(t.E, 256, 4096)), dim3(256), 0, st, k);
    TGMX_CHECK_LAUNCH("dos_large_estimate(keys)");
    if (rocprim::radix_sort_keys(pl.temp, pl.temp_bytes, (const u64*)pl.k_in, a.keys, (size_t)a.nmax, 0u, (unsigned)(2 * kDlCb + 1), st) != hipSuccess) {
      set_error("dos_large_estimate: radix sort failed");
      return TGMX_E_LAUNCH;
    }
  }
  hipLaunchKernelGGL(dos_large_count_kernel, tiles, wg, 0, st, a);
  TGMX_CHECK_LAUNCH("dos_large_estimate(count)");
  hipLaunchKernelGGL(dos_large_scan_kernel, dim3(1), wg, 0, st, (const u64*)a.blk_cnt, a.blk_base, pl.tiles, a.head, (int)kDlNnz, (int)kDlN, a.indptr);
  TGMX_CHECK_LAUNCH("dos_large_estimate(scan)");
  hipLaunchKernelGGL(dos_large_scatter_kernel, tiles, wg, 0, st, a);
  TGMX_CHECK_LAUNCH("dos_large_estimate(scatter)");
  hipLaunchKernelGGL(dos_large_entries_kernel, tiles, wg, 0, st, a);
  TGMX_CHECK_LAUNCH("dos_large_estimate(entries)");
  hipLaunchKernelGGL(dos_large_scan_kernel, dim3(1), wg, 0, st, (const u64*)a.blk_cnt, a.blk_base, pl.tiles, a.head, (int)kDlNSplit, (int)kDlNChunks,
                     (int*)nullptr);
  TGMX_CHECK_LAUNCH("dos_large_estimate(scan of long rows)");
  hipLaunchKernelGGL(dos_large_chunks_kernel, tiles, wg, 0, st, a);
  TGMX_CHECK_LAUNCH("dos_large_estimate(chunks)");

  const dim3 grid((unsigned)pl.groups);
  static std::atomic<bool> mom_attr[4][64];
#define TGMX_DOS_LARGE_MOMENTS(pv, slot)                                                                                  \
  do {                                                                                                                    \
    if (!dos_reserve_lds(dos_large_moments_kernel<pv>, mom_attr[slot], kDlLdsBytes)) return TGMX_E_LAUNCH;                \
    hipLaunchKernelGGL(dos_large_moments_kernel<pv>, grid, wg, kDlLdsBytes, st, a);                                       \
  } while (0)
  switch (a.PV) {
    case 8: TGMX_DOS_LARGE_MOMENTS(8, 0); break;
    case 4: TGMX_DOS_LARGE_MOMENTS(4, 1); break;
    case 2: TGMX_DOS_LARGE_MOMENTS(2, 2); break;
    default: TGMX_DOS_LARGE_MOMENTS(1, 3); break;
  }
#undef TGMX_DOS_LARGE_MOMENTS
  TGMX_CHECK_LAUNCH("dos_large_estimate(moments)");

  hipLaunchKernelGGL(dos_finish_kernel<DosLargeArgs>, dim3(1), dim3(kDosFinishThreads), 0, st, a);
  TGMX_CHECK_LAUNCH("dos_large_estimate(finish)");
  return TGMX_OK;
}
