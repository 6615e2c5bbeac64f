// The sorted-key CSR builder the sparse operators share (gcn.hip: GCN's normalised adjacency; cheb.hip: ChebConv's scaled Laplacian; ncn.hip:
// TNCN's symmetric adjacency).  An edge list becomes a CSR by row in four steps:
//   1. keys: every entry is one 64-bit key (row << cb | col), cb = bits of N; an entry its builder drops gets THE key behind every row,
//      1 << 2 cb.  Which entries are dropped, and what else the keys kernel leaves behind, is each builder's own.
//   2. ONE rocPRIM radix sort of the keys over the bits [0, 2 cb + 1), stable, the 32-bit edge positions riding along where the entries carry
//      values (equal keys then keep their edge order: the order of every later sum is fixed by the input alone).
//   3. row pointers: indptr[i] = the lower bound of (i << cb) in the sorted keys, a binary search per node (no scan, no atomics).
//   4. entries: cols[t] = the key's column; what else is stored per entry is the builder's functor.
// Nothing here adds floats with atomics: two runs give the same bits.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

namespace tgmx {

static int col_bits(long long N) {
  int cb = 1;
  while ((1ll << cb) < N) ++cb;
  return cb;
}

static unsigned grid_for(long long items, int per_block, long long cap) {
  long long blocks = (items + per_block - 1) / per_block;
  return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

// ---- keys ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long key_behind(int cb) { return 1ull << (2 * cb); }  // sorts behind every row
__device__ __forceinline__ unsigned long long key_row_start(long long row, int cb) { return (unsigned long long)row << cb; }
__device__ __forceinline__ unsigned long long key_of(bool keep, long long row, long long col, int cb) {
  return keep ? key_row_start(row, cb) | (unsigned long long)col : key_behind(cb);
}
__device__ __forceinline__ long long key_col(unsigned long long key, int cb) { return (long long)(key & ((1ull << cb) - 1)); }
__device__ __forceinline__ long long key_row(unsigned long long key, int cb) { return (long long)(key >> cb); }

// the first of the n sorted keys that is not below `want`
template <typename Key>
__device__ __forceinline__ long long key_lower_bound(const Key* __restrict__ sorted, long long n, Key want) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (sorted[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- the sort: 64-bit keys carrying 32-bit edge positions ---------------------------------------------------------------------------------
// (templates only so that a file that sorts keys alone, ncn.hip, does not instantiate the pair sort's kernels; Pos is unsigned)
template <typename Pos = unsigned>
static hipError_t sort_keys_pos_temp_bytes(size_t n, size_t& bytes) {
  bytes = 0;
  return rocprim::radix_sort_pairs(nullptr, bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const Pos*)nullptr, (Pos*)nullptr,
                                   n, 0u, 64u);
}
template <typename Pos = unsigned>
static hipError_t sort_keys_pos(void* temp, size_t temp_bytes, const unsigned long long* keys_in, unsigned long long* keys_out, const Pos* pos_in,
                                Pos* pos_out, size_t n, int cb, hipStream_t st) {
  return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, pos_in, pos_out, n, 0u, (unsigned)(2 * cb + 1), st);
}

// ---- rows ---------------------------------------------------------------------------------------------------------------------------------
// cols[t] of every sorted key and indptr[0 .. N]; `entry(t, col, row)` stores what else the builder keeps of entry t (called for the keys of
// the rows only, not for the ones behind them)
struct NoEntryValue {
  __device__ __forceinline__ void operator()(long long, long long, long long) const {}
};
template <typename Entry>
__global__ __launch_bounds__(256) void csr_rows_kernel(const unsigned long long* __restrict__ sorted, long long n, long long N, int cb,
                                                       int32_t* __restrict__ indptr, int32_t* __restrict__ cols, Entry entry) {
  const long long step = (long long)gridDim.x * blockDim.x;
  const long long total = n > N + 1 ? n : N + 1;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
    if (t < n) {
      const unsigned long long key = sorted[t];
      const long long col = key_col(key, cb);
      cols[t] = (int32_t)col;
      if (key < key_behind(cb)) entry(t, col, key_row(key, cb));
    }
    if (t <= N) indptr[t] = (int32_t)key_lower_bound(sorted, n, key_row_start(t, cb));
  }
}
template <typename Entry>
static void csr_rows_launch(const unsigned long long* sorted, long long n, long long N, int cb, int32_t* indptr, int32_t* cols, Entry entry,
                            hipStream_t st) {
  hipLaunchKernelGGL(csr_rows_kernel<Entry>, dim3(grid_for(n > N + 1 ? n : N + 1, 256, 4096)), dim3(256), 0, st, sorted, n, N, cb, indptr, cols, entry);
}

// ---- workspace ----------------------------------------------------------------------------------------------------------------------------
// Regions of a caller's workspace, taken in order, each on the 256-byte grid.  A builder walks the same sequence of take() calls twice:
// over no workspace to learn total(), over the caller's pointer to get the regions.  total() keeps 256 bytes of slack for aligning the base.
class WorkspaceCarver {
 public:
  explicit WorkspaceCarver(void* workspace) : base_(reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255)), live_(workspace != nullptr) {}
  template <typename T>
  T* take(size_t count) {
    T* p = live_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
    off_ = (off_ + count * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
  size_t total() const { return off_ + 256; }

 private:
  char* base_;
  bool live_;
  size_t off_ = 0;
};

}  // namespace tgmx
