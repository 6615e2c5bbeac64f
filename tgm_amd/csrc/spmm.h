// The gather SpMM the sparse propagations share (cheb.hip: the scaled Laplacian of ChebConv; gcn.hip: GCN's normalised adjacency; the CSR
// comes from edge_csr.h).  out[i] = epi(i, diag[i] t[i] + sum_{j in row i} vals[j] t[cols[j]]) over a CSR by destination.
//
// A workgroup of four waves owns four destination rows; a wave walks its row's entries four at a time (four source rows requested before the
// first is used), the lanes spread over the channels.  A row of more than kSpmmLongRow entries is cut into four contiguous pieces, one per
// wave, and the partial sums meet in LDS in wave order.  A row of more than kSpmmVeryLong entries (a hub: the most popular page of a
// wiki-shaped day has 21 000) would still keep one workgroup busy long after the others have left, so the caller's scratch takes it out of
// that launch: a second launch cuts the ENTRY array into chunks of kSpmmChunk, a workgroup per chunk sums the part of the (at most two) very
// long rows its chunk holds, and a third adds a row's chunk sums in ascending chunk order.  Every order is fixed by the CSR alone.
//
// The epilogue is a template parameter, a struct carried by value in the kernel's arguments with
//   template <bool VEC> __device__ void apply(long long i, int c0, int C, int lane, float o[kSpmmChPerLane]) const
// which turns a row's sums of one channel pass into what is stored (o holds diag[i] t[i] + the gathered sum on entry).  It runs wherever a
// row finishes: the short row, wave 0 of a long row, the join kernel.
//
// An epilogue that declares `static constexpr bool kGatherOnly = true` makes the propagation a plain row gather (decoder_bwd.hip: the
// scatter of the pair gradients, read back through the inverted index): every value is 1 (vals is not read: acc += x), there is no
// diagonal term (diag and t[i] are not read: out has other rows than t), apply() is not called, and row i is stored at
//   __device__ float* row(float* out, long long ldo, long long i) const
#pragma once
#include <type_traits>

#include "common.h"

namespace tgmx {

constexpr int kSpmmThreads = 256;
constexpr int kSpmmWaves = kSpmmThreads / kWave;
constexpr int kSpmmLongRow = 64;   // entries; longer rows are split over the workgroup's waves
constexpr int kSpmmChPerLane = 4;  // channels a lane covers per pass: 256 channels a pass
constexpr int kSpmmChunk = 1024;   // entries of the CSR one workgroup of the chunk launch covers
constexpr int kSpmmVeryLong = 2 * kSpmmChunk;  // rows longer than this go through the chunk launch: a chunk then meets at most two of them

// a lane's channels of one pass: VEC: the float4 at c0 + 4 lane;  else c0 + lane + 64 q, q < 4
template <bool VEC>
__device__ __forceinline__ void spmm_load(const float* __restrict__ row, int c0, int C, int lane, float x[kSpmmChPerLane]) {
  if (VEC) {
    const int c = c0 + lane * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < C) v = *reinterpret_cast<const float4*>(row + c);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  } else {
#pragma unroll
    for (int q = 0; q < kSpmmChPerLane; ++q) {
      const int c = c0 + lane + q * kWave;
      x[q] = c < C ? row[c] : 0.f;
    }
  }
}
template <bool VEC>
__device__ __forceinline__ void spmm_store(float* __restrict__ row, int c0, int C, int lane, const float x[kSpmmChPerLane]) {
  if (VEC) {
    const int c = c0 + lane * 4;
    if (c < C) *reinterpret_cast<float4*>(row + c) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
#pragma unroll
    for (int q = 0; q < kSpmmChPerLane; ++q) {
      const int c = c0 + lane + q * kWave;
      if (c < C) row[c] = x[q];
    }
  }
}

template <typename Epi, typename = void>
struct spmm_gather_only : std::false_type {};
template <typename Epi>
struct spmm_gather_only<Epi, std::void_t<decltype(Epi::kGatherOnly)>> : std::bool_constant<Epi::kGatherOnly> {};

// acc += sum over the entries [lo, hi) in ascending order, four source rows requested ahead (UNIT: every value is 1)
template <bool VEC, bool UNIT = false>
__device__ __forceinline__ void spmm_accumulate(const int32_t* __restrict__ cols, const float* __restrict__ vals, int lo, int hi,
                                                const float* __restrict__ t, long long ldt, int c0, int C, int lane, float acc[kSpmmChPerLane]) {
  int j = lo;
  for (; j + 4 <= hi; j += 4) {
    float x[4][kSpmmChPerLane], v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[u] = UNIT ? 1.f : vals[j + u];
      spmm_load<VEC>(t + (long long)cols[j + u] * ldt, c0, C, lane, x[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int q = 0; q < kSpmmChPerLane; ++q) acc[q] = UNIT ? __fadd_rn(acc[q], x[u][q]) : __fmaf_rn(v[u], x[u][q], acc[q]);
  }
  for (; j < hi; ++j) {
    float x[kSpmmChPerLane];
    const float v = UNIT ? 1.f : vals[j];
    spmm_load<VEC>(t + (long long)cols[j] * ldt, c0, C, lane, x);
#pragma unroll
    for (int q = 0; q < kSpmmChPerLane; ++q) acc[q] = UNIT ? __fadd_rn(acc[q], x[q]) : __fmaf_rn(v, x[q], acc[q]);
  }
}

template <typename Epi>
struct SpmmArgs {
  const int32_t* indptr;
  const int32_t* cols;
  const float* vals;
  const float* diag;
  long long N;
  int C;
  const float* t;
  long long ldt;
  float* out;
  long long ldo;
  int very_long;   // rows longer than this are left to the chunk launches
  float* scratch;  // [chunks, 2, C]: the chunk launches' partial sums
  Epi epi;
};

// out row i of one channel pass from the gathered sum acc
template <bool VEC, typename Epi>
__device__ __forceinline__ void spmm_finish(const SpmmArgs<Epi>& a, long long i, int c0, int lane, float acc[kSpmmChPerLane]) {
  if constexpr (spmm_gather_only<Epi>::value) {
    spmm_store<VEC>(a.epi.row(a.out, a.ldo, i), c0, a.C, lane, acc);
  } else {
    float self[kSpmmChPerLane], o[kSpmmChPerLane];
    spmm_load<VEC>(a.t + i * a.ldt, c0, a.C, lane, self);
    const float d = a.diag[i];
#pragma unroll
    for (int q = 0; q < kSpmmChPerLane; ++q) o[q] = __fmaf_rn(d, self[q], acc[q]);
    a.epi.template apply<VEC>(i, c0, a.C, lane, o);
    spmm_store<VEC>(a.out + i * a.ldo, c0, a.C, lane, o);
  }
}

// the sum over the entries [lo, hi) by the four waves of a workgroup, a contiguous quarter each, the partial sums added in wave order: the
// total in wave 0's acc.  Called by every thread of the workgroup with the same bounds (two barriers).
template <bool VEC, typename Epi>
__device__ __forceinline__ void spmm_block_sum(const SpmmArgs<Epi>& a, int lo, int hi, int c0, int lane, int wave,
                                               float (*part)[kSpmmChPerLane][kWave], float acc[kSpmmChPerLane]) {
  const int piece = (hi - lo + kSpmmWaves - 1) / kSpmmWaves;
  const int mylo = min(lo + wave * piece, hi), myhi = min(mylo + piece, hi);
#pragma unroll
  for (int q = 0; q < kSpmmChPerLane; ++q) acc[q] = 0.f;
  spmm_accumulate<VEC, spmm_gather_only<Epi>::value>(a.cols, a.vals, mylo, myhi, a.t, a.ldt, c0, a.C, lane, acc);
#pragma unroll
  for (int q = 0; q < kSpmmChPerLane; ++q) part[wave][q][lane] = acc[q];
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int q = 0; q < kSpmmChPerLane; ++q) {
      float s = part[0][q][lane];
#pragma unroll
      for (int w = 1; w < kSpmmWaves; ++w) s += part[w][q][lane];
      acc[q] = s;
    }
  }
  __syncthreads();
}

template <bool VEC, typename Epi>
__global__ __launch_bounds__(kSpmmThreads) void spmm_propagate_kernel(SpmmArgs<Epi> a) {
  __shared__ float part[kSpmmWaves][kSpmmChPerLane][kWave];
  const int lane = lane_id(), wave = threadIdx.x / kWave;
  const long long row0 = (long long)blockIdx.x * kSpmmWaves;
  // short rows: one wave each
  {
    const long long i = row0 + wave;
    if (i < a.N) {
      const int lo = a.indptr[i], hi = a.indptr[i + 1];
      if (hi - lo <= kSpmmLongRow) {
        for (int c0 = 0; c0 < a.C; c0 += kWave * kSpmmChPerLane) {
          float acc[kSpmmChPerLane] = {0.f, 0.f, 0.f, 0.f};
          spmm_accumulate<VEC, spmm_gather_only<Epi>::value>(a.cols, a.vals, lo, hi, a.t, a.ldt, c0, a.C, lane, acc);
          spmm_finish<VEC>(a, i, c0, lane, acc);
        }
      }
    }
  }
  // long rows: the four waves take a contiguous quarter each (every thread of the workgroup sees the same lengths: the barriers are uniform)
  for (int r = 0; r < kSpmmWaves; ++r) {
    const long long i = row0 + r;
    if (i >= a.N) break;
    const int lo = a.indptr[i], hi = a.indptr[i + 1];
    if (hi - lo <= kSpmmLongRow || hi - lo > a.very_long) continue;
    for (int c0 = 0; c0 < a.C; c0 += kWave * kSpmmChPerLane) {
      float acc[kSpmmChPerLane];
      spmm_block_sum<VEC>(a, lo, hi, c0, lane, wave, part, acc);
      if (wave == 0) spmm_finish<VEC>(a, i, c0, lane, acc);
    }
  }
}

// the row that holds entry e < indptr[N]
__device__ __forceinline__ int spmm_row_of(const int32_t* __restrict__ indptr, int N, int e) {
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = (int)(((long long)lo + hi) >> 1);
    if (indptr[mid + 1] <= e) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// chunk b of the entry array: the partial sums of the very long rows that hold its first entry (slot 0) and its last entry (slot 1)
template <bool VEC, typename Epi>
__global__ __launch_bounds__(kSpmmThreads) void spmm_chunk_kernel(SpmmArgs<Epi> a) {
  __shared__ float part[kSpmmWaves][kSpmmChPerLane][kWave];
  const int lane = lane_id(), wave = threadIdx.x / kWave;
  const int N = (int)a.N, nnz = a.indptr[N];
  const long long e0l = (long long)blockIdx.x * kSpmmChunk;
  if (e0l >= nnz) return;
  const int e0 = (int)e0l, e1 = (int)(e0l + kSpmmChunk < nnz ? e0l + kSpmmChunk : nnz);
  const int rA = spmm_row_of(a.indptr, N, e0), rB = spmm_row_of(a.indptr, N, e1 - 1);
  for (int slot = 0; slot < 2; ++slot) {
    const int r = slot ? rB : rA;
    if (slot && rB == rA) break;
    const int lo = a.indptr[r], hi = a.indptr[r + 1];
    if (hi - lo <= a.very_long) continue;
    const int slo = lo > e0 ? lo : e0, shi = hi < e1 ? hi : e1;
    float* __restrict__ dst = a.scratch + ((long long)blockIdx.x * 2 + slot) * a.C;
    for (int c0 = 0; c0 < a.C; c0 += kWave * kSpmmChPerLane) {
      float acc[kSpmmChPerLane];
      spmm_block_sum<VEC>(a, slo, shi, c0, lane, wave, part, acc);
      if (wave == 0) spmm_store<VEC>(dst, c0, a.C, lane, acc);
    }
  }
}

// a very long row: its chunks' partial sums in ascending chunk order, then the row's epilogue; one wave per row
template <bool VEC, typename Epi>
__global__ __launch_bounds__(kSpmmThreads) void spmm_join_kernel(SpmmArgs<Epi> a) {
  const int lane = lane_id();
  const long long i = (long long)blockIdx.x * kSpmmWaves + threadIdx.x / kWave;
  if (i >= a.N) return;
  const int lo = a.indptr[i], hi = a.indptr[i + 1];
  if (hi - lo <= a.very_long) return;
  for (int c0 = 0; c0 < a.C; c0 += kWave * kSpmmChPerLane) {
    float acc[kSpmmChPerLane] = {0.f, 0.f, 0.f, 0.f};
    for (int b = lo / kSpmmChunk; b <= (hi - 1) / kSpmmChunk; ++b) {
      const int slot = b * kSpmmChunk >= lo ? 0 : 1;  // the row holds the chunk's first entry, or it starts inside the chunk and holds its last
      float x[kSpmmChPerLane];
      spmm_load<VEC>(a.scratch + ((long long)b * 2 + slot) * a.C, c0, a.C, lane, x);
#pragma unroll
      for (int q = 0; q < kSpmmChPerLane; ++q) acc[q] += x[q];
    }
    spmm_finish<VEC>(a, i, c0, lane, acc);
  }
}

static inline size_t spmm_scratch_floats(long long nnz, int C) {
  if (nnz <= kSpmmVeryLong || C <= 0) return 0;  // no row can be very long
  return (size_t)((nnz + kSpmmChunk - 1) / kSpmmChunk) * 2 * (size_t)C;
}

static inline bool spmm_vec_ok(const float* p, long long ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

// The one, two or three launches of a propagation.  a.very_long / a.scratch are set here: very long rows leave the first launch only when
// the caller brought the scratch for their chunk sums.  `vec`: every operand the kernels touch besides the scratch is on the 16-byte grid.
template <typename Epi>
static int spmm_run(SpmmArgs<Epi> a, long long nnz, float* scratch, size_t scratch_floats, bool vec, const char* what, hipStream_t st) {
  const size_t need = spmm_scratch_floats(nnz, a.C);
  const bool chunks = need > 0 && scratch != nullptr;
  if (chunks && scratch_floats < need) {
    set_error("%s: scratch too small (%zu floats, %zu needed)", what, scratch_floats, need);
    return TGMX_E_INVALID;
  }
  a.very_long = chunks ? kSpmmVeryLong : 0x7fffffff;
  a.scratch = chunks ? scratch : nullptr;
  vec = vec && a.C % 4 == 0 && (!chunks || spmm_vec_ok(scratch, 4));
  const dim3 grid((unsigned)((a.N + kSpmmWaves - 1) / kSpmmWaves)), block(kSpmmThreads);
  if (vec) hipLaunchKernelGGL((spmm_propagate_kernel<true, Epi>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((spmm_propagate_kernel<false, Epi>), grid, block, 0, st, a);
  TGMX_CHECK_LAUNCH(what);
  if (chunks) {
    const dim3 cgrid((unsigned)((nnz + kSpmmChunk - 1) / kSpmmChunk));
    if (vec) hipLaunchKernelGGL((spmm_chunk_kernel<true, Epi>), cgrid, block, 0, st, a);
    else hipLaunchKernelGGL((spmm_chunk_kernel<false, Epi>), cgrid, block, 0, st, a);
    TGMX_CHECK_LAUNCH(what);
    if (vec) hipLaunchKernelGGL((spmm_join_kernel<true, Epi>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((spmm_join_kernel<false, Epi>), grid, block, 0, st, a);
    TGMX_CHECK_LAUNCH(what);
  }
  return TGMX_OK;
}

}  // namespace tgmx
