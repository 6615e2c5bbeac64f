// ChebConv and the GCLSTM cell (the reference's tgm/nn/encoder/gclstm.py) for gfx950: the scaled Laplacian of a snapshot as a CSR by
// destination, a gather SpMM over it, the LSTM gate epilogue, and the cell's inference forward as one call.  ChebConv is third-party to the
// reference (torch_geometric); it is implemented from its published definition (get_laplacian, then 2 L / lambda_max - I): parity unpinned
// upstream.
//
// Laplacian: the E edges become keys (dst << cb | src), cb = bits of N, carrying their edge position through ONE stable radix sort
// (rocPRIM); a self loop or an edge with an endpoint outside [0, N) gets a key behind every row.  Row pointers are a binary search per node
// (no scan, no atomics).  The degree is taken over the SOURCE index: without weights it is an integer count (integer atomics do not depend
// on the order of arrival); with weights a second stable sort by source groups the positions and one wave per node sums its group in a
// fixed order.  Nothing here adds floats with atomics: two runs give the same bits.
//
// Propagate: out = alpha (L_hat t) + beta prev, gather form.  A workgroup of four waves owns four destination rows; a wave walks its row's
// entries four at a time (four source rows requested before the first is used), the lanes spread over the channels.  A row of more than
// kChebLongRow entries is cut into four contiguous pieces, one per wave, and the partial sums meet in LDS in wave order.  A row of more than
// kChebVeryLong entries (a hub: the most popular page of a wiki-shaped day has 21 000) would still keep one workgroup busy long after the
// others have left, so the caller's scratch takes it out of that launch: a second launch cuts the ENTRY array into chunks of kChebChunk, a
// workgroup per chunk sums the part of the (at most two) very long rows its chunk holds, and a third adds a row's chunk sums in ascending
// chunk order.  Every order is fixed by the CSR alone.
#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

namespace tgmx {

constexpr int kChebThreads = 256;
constexpr int kChebWaves = kChebThreads / kWave;
constexpr int kChebLongRow = 64;   // entries; longer rows are split over the workgroup's waves
constexpr int kChebChPerLane = 4;  // channels a lane covers per pass: 256 channels a pass
constexpr int kChebChunk = 1024;   // entries of the CSR one workgroup of the chunk launch covers
constexpr int kChebVeryLong = 2 * kChebChunk;  // rows longer than this go through the chunk launch: a chunk then meets at most two of them

__device__ __forceinline__ long long cheb_idx(const void* p, int is64, long long i) {
  return is64 ? (long long)reinterpret_cast<const int64_t*>(p)[i] : (long long)reinterpret_cast<const int32_t*>(p)[i];
}

static int cheb_col_bits(long long N) {
  int cb = 1;
  while ((1ll << cb) < N) ++cb;
  return cb;
}

static unsigned cheb_grid(long long items, int per_block, long long cap) {
  long long blocks = (items + per_block - 1) / per_block;
  return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

// ---- Laplacian --------------------------------------------------------------------------------------------------------------------------
// keys by destination (and by source when the degrees are weighted); cnt: the unweighted degree as an integer count
__global__ __launch_bounds__(256) void cheb_keys_kernel(const void* __restrict__ src, const void* __restrict__ dst, int is64, long long E, long long N,
                                                        int cb, unsigned long long* __restrict__ kd, unsigned* __restrict__ pos,
                                                        unsigned* __restrict__ ks, int* __restrict__ cnt, int* __restrict__ skipped) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += step) {
    const long long s = cheb_idx(src, is64, e), d = cheb_idx(dst, is64, e);
    const bool in = s >= 0 && s < N && d >= 0 && d < N;
    const bool ok = in && s != d;
    if (!in && skipped) atomicAdd(skipped, 1);
    kd[e] = ok ? ((unsigned long long)d << cb) | (unsigned long long)s : 1ull << (2 * cb);  // sorts behind every row
    pos[e] = (unsigned)e;
    if (ks) ks[e] = ok ? (unsigned)s : (unsigned)N;
    else if (ok) atomicAdd(&cnt[s], 1);
  }
}

// dis[i]: the factor the normalisation takes from node i's degree (deg^-1/2, 1/deg, or the degree itself for NONE); diag[i]
// One wave per node: with weights the lanes stride over the node's group of the source-sorted positions and the partial sums are folded
// in a fixed butterfly.
__global__ __launch_bounds__(kChebThreads) void cheb_degree_kernel(const unsigned* __restrict__ ks_sorted, const unsigned* __restrict__ ps_sorted,
                                                                   const float* __restrict__ w, const int* __restrict__ cnt, long long E, long long N,
                                                                   int norm, float lambda_max, const float* __restrict__ lambda_ptr,
                                                                   float* __restrict__ dis, float* __restrict__ diag) {
  const int lane = lane_id();
  const long long nwaves = (long long)gridDim.x * kChebWaves;
  const float lmax = lambda_ptr ? lambda_ptr[0] : lambda_max;
  for (long long i = (long long)blockIdx.x * kChebWaves + threadIdx.x / kWave; i < N; i += nwaves) {
    float deg;
    if (ks_sorted) {
      long long lo = 0, hi = E;
      while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long)ks_sorted[mid] < i) lo = mid + 1;
        else hi = mid;
      }
      long long end = lo;
      hi = E;
      while (end < hi) {
        const long long mid = (end + hi) >> 1;
        if ((long long)ks_sorted[mid] <= i) end = mid + 1;
        else hi = mid;
      }
      float part = 0.f;
      for (long long j = lo + lane; j < end; j += kWave) part += w[ps_sorted[j]];
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) part += __shfl_xor(part, off);
      deg = part;
    } else {
      deg = (float)cnt[i];
    }
    if (lane == 0) {
      float f, d = 1.f;
      if (norm == TGMX_CHEB_NORM_SYM) {
        f = 1.0f / sqrtf(deg);
        if (isinf(f)) f = 0.f;
      } else if (norm == TGMX_CHEB_NORM_RW) {
        f = 1.0f / deg;
        if (isinf(f)) f = 0.f;
      } else {
        f = deg;
        d = deg;
      }
      dis[i] = f;
      float dv = (2.0f * d) / lmax;
      if (isinf(dv)) dv = 0.f;
      diag[i] = dv - 1.0f;
    }
  }
}

__global__ __launch_bounds__(256) void cheb_rows_kernel(const unsigned long long* __restrict__ sorted, const unsigned* __restrict__ pos_sorted,
                                                        const float* __restrict__ w, const float* __restrict__ dis, long long E, long long N, int cb,
                                                        int norm, float lambda_max, const float* __restrict__ lambda_ptr,
                                                        int32_t* __restrict__ indptr, int32_t* __restrict__ cols, float* __restrict__ vals) {
  const long long step = (long long)gridDim.x * blockDim.x;
  const long long total = E > N + 1 ? E : N + 1;
  const float lmax = lambda_ptr ? lambda_ptr[0] : lambda_max;
  const unsigned long long behind = 1ull << (2 * cb);
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
    if (t < E) {
      const unsigned long long key = sorted[t];
      if (key < behind) {
        const long long s = (long long)(key & ((1ull << cb) - 1)), d = (long long)(key >> cb);
        const float we = w ? w[pos_sorted[t]] : 1.f;
        float m;
        if (norm == TGMX_CHEB_NORM_SYM) m = dis[s] * we * dis[d];
        else if (norm == TGMX_CHEB_NORM_RW) m = dis[s] * we;
        else m = we;
        float v = (2.0f * -m) / lmax;
        if (isinf(v)) v = 0.f;
        cols[t] = (int32_t)s;
        vals[t] = v;
      }
    }
    if (t <= N) {
      const unsigned long long want = (unsigned long long)t << cb;
      long long lo = 0, hi = E;
      while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (sorted[mid] < want) lo = mid + 1;
        else hi = mid;
      }
      indptr[t] = (int32_t)lo;
    }
  }
}

struct ChebLayout {
  size_t kd_in, kd_out, pos_in, pos_out, ks_in, ks_out, ps_out, cnt, dis, temp, temp_bytes, total;
};
static int cheb_layout(long long E, long long N, ChebLayout& w) {
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t n = (size_t)(E > 0 ? E : 1);
  size_t off = 0;
  w.kd_in = off; off = up(off + n * 8);
  w.kd_out = off; off = up(off + n * 8);
  w.pos_in = off; off = up(off + n * 4);
  w.pos_out = off; off = up(off + n * 4);
  w.ks_in = off; off = up(off + n * 4);
  w.ks_out = off; off = up(off + n * 4);
  w.ps_out = off; off = up(off + n * 4);
  w.cnt = off; off = up(off + (size_t)N * 4);
  w.dis = off; off = up(off + (size_t)N * 4);
  size_t tb64 = 0, tb32 = 0;
  if (rocprim::radix_sort_pairs(nullptr, tb64, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const unsigned*)nullptr,
                                (unsigned*)nullptr, n, 0u, 64u) != hipSuccess)
    return TGMX_E_LAUNCH;
  if (rocprim::radix_sort_pairs(nullptr, tb32, (const unsigned*)nullptr, (unsigned*)nullptr, (const unsigned*)nullptr, (unsigned*)nullptr, n, 0u,
                                32u) != hipSuccess)
    return TGMX_E_LAUNCH;
  w.temp = off; w.temp_bytes = tb64 > tb32 ? tb64 : tb32; off = up(off + w.temp_bytes);
  w.total = off + 256;
  return TGMX_OK;
}

// ---- propagate ----------------------------------------------------------------------------------------------------------------------------
// a lane's channels of one pass: VEC: the float4 at c0 + 4 lane;  else c0 + lane + 64 q, q < 4
template <bool VEC>
__device__ __forceinline__ void cheb_load(const float* __restrict__ row, int c0, int C, int lane, float x[kChebChPerLane]) {
  if (VEC) {
    const int c = c0 + lane * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < C) v = *reinterpret_cast<const float4*>(row + c);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  } else {
#pragma unroll
    for (int q = 0; q < kChebChPerLane; ++q) {
      const int c = c0 + lane + q * kWave;
      x[q] = c < C ? row[c] : 0.f;
    }
  }
}
template <bool VEC>
__device__ __forceinline__ void cheb_store(float* __restrict__ row, int c0, int C, int lane, const float x[kChebChPerLane]) {
  if (VEC) {
    const int c = c0 + lane * 4;
    if (c < C) *reinterpret_cast<float4*>(row + c) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
#pragma unroll
    for (int q = 0; q < kChebChPerLane; ++q) {
      const int c = c0 + lane + q * kWave;
      if (c < C) row[c] = x[q];
    }
  }
}

// acc += sum over the entries [lo, hi) in ascending order, four source rows requested ahead
template <bool VEC>
__device__ __forceinline__ void cheb_accumulate(const int32_t* __restrict__ cols, const float* __restrict__ vals, int lo, int hi,
                                                const float* __restrict__ t, long long ldt, int c0, int C, int lane, float acc[kChebChPerLane]) {
  int j = lo;
  for (; j + 4 <= hi; j += 4) {
    float x[4][kChebChPerLane], v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[u] = vals[j + u];
      cheb_load<VEC>(t + (long long)cols[j + u] * ldt, c0, C, lane, x[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int q = 0; q < kChebChPerLane; ++q) acc[q] = __fmaf_rn(v[u], x[u][q], acc[q]);
  }
  for (; j < hi; ++j) {
    float x[kChebChPerLane];
    const float v = vals[j];
    cheb_load<VEC>(t + (long long)cols[j] * ldt, c0, C, lane, x);
#pragma unroll
    for (int q = 0; q < kChebChPerLane; ++q) acc[q] = __fmaf_rn(v, x[q], acc[q]);
  }
}

struct ChebProp {
  const int32_t* indptr;
  const int32_t* cols;
  const float* vals;
  const float* diag;
  long long N;
  int C;
  const float* t;
  long long ldt;
  const float* prev;
  long long ldp;
  float alpha, beta;
  float* out;
  long long ldo;
  int very_long;   // rows longer than this are left to the chunk launches
  float* scratch;  // [chunks, 2, C]: the chunk launches' partial sums
};

// out row i of one channel pass from the gathered sum acc
template <bool VEC>
__device__ __forceinline__ void cheb_finish(const ChebProp& a, long long i, int c0, int lane, float acc[kChebChPerLane]) {
  float self[kChebChPerLane], o[kChebChPerLane];
  cheb_load<VEC>(a.t + i * a.ldt, c0, a.C, lane, self);
  const float d = a.diag[i];
#pragma unroll
  for (int q = 0; q < kChebChPerLane; ++q) o[q] = a.alpha * __fmaf_rn(d, self[q], acc[q]);
  if (a.beta != 0.f) {
    float p[kChebChPerLane];
    cheb_load<VEC>(a.prev + i * a.ldp, c0, a.C, lane, p);
#pragma unroll
    for (int q = 0; q < kChebChPerLane; ++q) o[q] = __fmaf_rn(a.beta, p[q], o[q]);
  }
  cheb_store<VEC>(a.out + i * a.ldo, c0, a.C, lane, o);
}

// the sum over the entries [lo, hi) by the four waves of a workgroup, a contiguous quarter each, the partial sums added in wave order: the
// total in wave 0's acc.  Called by every thread of the workgroup with the same bounds (two barriers).
template <bool VEC>
__device__ __forceinline__ void cheb_block_sum(const ChebProp& a, int lo, int hi, int c0, int lane, int wave,
                                               float (*part)[kChebChPerLane][kWave], float acc[kChebChPerLane]) {
  const int piece = (hi - lo + kChebWaves - 1) / kChebWaves;
  const int mylo = min(lo + wave * piece, hi), myhi = min(mylo + piece, hi);
#pragma unroll
  for (int q = 0; q < kChebChPerLane; ++q) acc[q] = 0.f;
  cheb_accumulate<VEC>(a.cols, a.vals, mylo, myhi, a.t, a.ldt, c0, a.C, lane, acc);
#pragma unroll
  for (int q = 0; q < kChebChPerLane; ++q) part[wave][q][lane] = acc[q];
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int q = 0; q < kChebChPerLane; ++q) {
      float s = part[0][q][lane];
#pragma unroll
      for (int w = 1; w < kChebWaves; ++w) s += part[w][q][lane];
      acc[q] = s;
    }
  }
  __syncthreads();
}

template <bool VEC>
__global__ __launch_bounds__(kChebThreads) void cheb_propagate_kernel(ChebProp a) {
  __shared__ float part[kChebWaves][kChebChPerLane][kWave];
  const int lane = lane_id(), wave = threadIdx.x / kWave;
  const long long row0 = (long long)blockIdx.x * kChebWaves;
  // short rows: one wave each
  {
    const long long i = row0 + wave;
    if (i < a.N) {
      const int lo = a.indptr[i], hi = a.indptr[i + 1];
      if (hi - lo <= kChebLongRow) {
        for (int c0 = 0; c0 < a.C; c0 += kWave * kChebChPerLane) {
          float acc[kChebChPerLane] = {0.f, 0.f, 0.f, 0.f};
          cheb_accumulate<VEC>(a.cols, a.vals, lo, hi, a.t, a.ldt, c0, a.C, lane, acc);
          cheb_finish<VEC>(a, i, c0, lane, acc);
        }
      }
    }
  }
  // long rows: the four waves take a contiguous quarter each (every thread of the workgroup sees the same lengths: the barriers are uniform)
  for (int r = 0; r < kChebWaves; ++r) {
    const long long i = row0 + r;
    if (i >= a.N) break;
    const int lo = a.indptr[i], hi = a.indptr[i + 1];
    if (hi - lo <= kChebLongRow || hi - lo > a.very_long) continue;
    for (int c0 = 0; c0 < a.C; c0 += kWave * kChebChPerLane) {
      float acc[kChebChPerLane];
      cheb_block_sum<VEC>(a, lo, hi, c0, lane, wave, part, acc);
      if (wave == 0) cheb_finish<VEC>(a, i, c0, lane, acc);
    }
  }
}

// the row that holds entry e < indptr[N]
__device__ __forceinline__ int cheb_row_of(const int32_t* __restrict__ indptr, int N, int e) {
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = (int)(((long long)lo + hi) >> 1);
    if (indptr[mid + 1] <= e) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// chunk b of the entry array: the partial sums of the very long rows that hold its first entry (slot 0) and its last entry (slot 1)
template <bool VEC>
__global__ __launch_bounds__(kChebThreads) void cheb_chunk_kernel(ChebProp a) {
  __shared__ float part[kChebWaves][kChebChPerLane][kWave];
  const int lane = lane_id(), wave = threadIdx.x / kWave;
  const int N = (int)a.N, nnz = a.indptr[N];
  const long long e0l = (long long)blockIdx.x * kChebChunk;
  if (e0l >= nnz) return;
  const int e0 = (int)e0l, e1 = (int)(e0l + kChebChunk < nnz ? e0l + kChebChunk : nnz);
  const int rA = cheb_row_of(a.indptr, N, e0), rB = cheb_row_of(a.indptr, N, e1 - 1);
  for (int slot = 0; slot < 2; ++slot) {
    const int r = slot ? rB : rA;
    if (slot && rB == rA) break;
    const int lo = a.indptr[r], hi = a.indptr[r + 1];
    if (hi - lo <= a.very_long) continue;
    const int slo = lo > e0 ? lo : e0, shi = hi < e1 ? hi : e1;
    float* __restrict__ dst = a.scratch + ((long long)blockIdx.x * 2 + slot) * a.C;
    for (int c0 = 0; c0 < a.C; c0 += kWave * kChebChPerLane) {
      float acc[kChebChPerLane];
      cheb_block_sum<VEC>(a, slo, shi, c0, lane, wave, part, acc);
      if (wave == 0) cheb_store<VEC>(dst, c0, a.C, lane, acc);
    }
  }
}

// a very long row: its chunks' partial sums in ascending chunk order, then the row's epilogue; one wave per row
template <bool VEC>
__global__ __launch_bounds__(kChebThreads) void cheb_join_kernel(ChebProp a) {
  const int lane = lane_id();
  const long long i = (long long)blockIdx.x * kChebWaves + threadIdx.x / kWave;
  if (i >= a.N) return;
  const int lo = a.indptr[i], hi = a.indptr[i + 1];
  if (hi - lo <= a.very_long) return;
  for (int c0 = 0; c0 < a.C; c0 += kWave * kChebChPerLane) {
    float acc[kChebChPerLane] = {0.f, 0.f, 0.f, 0.f};
    for (int b = lo / kChebChunk; b <= (hi - 1) / kChebChunk; ++b) {
      const int slot = b * kChebChunk >= lo ? 0 : 1;  // the row holds the chunk's first entry, or it starts inside the chunk and holds its last
      float x[kChebChPerLane];
      cheb_load<VEC>(a.scratch + ((long long)b * 2 + slot) * a.C, c0, a.C, lane, x);
#pragma unroll
      for (int q = 0; q < kChebChPerLane; ++q) acc[q] += x[q];
    }
    cheb_finish<VEC>(a, i, c0, lane, acc);
  }
}

// ---- the cell -------------------------------------------------------------------------------------------------------------------------------
// op[i, :in] = x[i], op[i, in : in + C] = H[i] (Tx_0), the padding columns [width, ldop) zero
__global__ __launch_bounds__(256) void gclstm_operand_kernel(const float* __restrict__ x, int in_ch, const float* __restrict__ H, int C, int width,
                                                             long long N, float* __restrict__ op, long long ldop) {
  const int fill = in_ch + C + (int)(ldop - width);  // columns written per row
  const long long total = N * fill;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += step) {
    const long long i = p / fill;
    const int c = (int)(p - i * fill);
    if (c < in_ch) op[i * ldop + c] = x[i * in_ch + c];
    else if (c < in_ch + C) op[i * ldop + c] = H[i * C + (c - in_ch)];
    else op[i * ldop + width + (c - in_ch - C)] = 0.f;
  }
}

// pre [N, 4C] = the pre-activations of the gates i, f, c, o:  C' = sigmoid(f) C + sigmoid(i) tanh(c),  H' = sigmoid(o) tanh(C')   (gclstm.py:165-227)
__global__ __launch_bounds__(256) void gclstm_gates_kernel(const float* __restrict__ pre, const float* __restrict__ Cprev, int C, long long N,
                                                           float* __restrict__ H_out, float* __restrict__ C_out) {
  const long long total = N * C;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += step) {
    const long long i = p / C;
    const int c = (int)(p - i * C);
    const float* g = pre + i * 4 * C + c;
    const float I = 1.f / (1.f + expf(-g[0]));
    const float F = 1.f / (1.f + expf(-g[C]));
    const float T = tanhf(g[2 * C]);
    const float O = 1.f / (1.f + expf(-g[3 * C]));
    const float cn = F * Cprev[p] + I * T;
    C_out[p] = cn;
    H_out[p] = O * tanhf(cn);
  }
}

}  // namespace tgmx

using namespace tgmx;

extern "C" size_t tgmx_cheb_workspace_bytes(int64_t E, int64_t N) {
  ChebLayout w;
  if (E < 0 || E >= (1ll << 31) || N <= 0 || N >= (1ll << 31)) return 0;
  return cheb_layout(E, N, w) == TGMX_OK ? w.total : 0;
}

extern "C" int tgmx_cheb_laplacian(const void* src, const void* dst, int32_t idx64, const float* w, int64_t E, int64_t N, int32_t normalization,
                                   float lambda_max, const float* lambda_ptr, int32_t* indptr, int32_t* cols, float* vals, float* diag,
                                   void* workspace, size_t workspace_bytes, int32_t* skipped, tgmx_stream_t stream) {
  TGMX_REQUIRE(E >= 0 && E < (1ll << 31) && N > 0 && N < (1ll << 31), "cheb_laplacian: bad sizes E=%lld N=%lld", (long long)E, (long long)N);
  TGMX_REQUIRE(normalization >= TGMX_CHEB_NORM_NONE && normalization <= TGMX_CHEB_NORM_RW, "cheb_laplacian: unknown normalization %d", normalization);
  TGMX_REQUIRE(indptr && diag && workspace && (E == 0 || (src && dst && cols && vals)), "cheb_laplacian: null pointer");
  hipStream_t st = (hipStream_t)stream;
  ChebLayout l;
  if (cheb_layout(E, N, l) != TGMX_OK || workspace_bytes < l.total) {
    set_error("cheb_laplacian: workspace too small (%zu bytes)", workspace_bytes);
    return TGMX_E_INVALID;
  }
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  auto* kd_in = reinterpret_cast<unsigned long long*>(base + l.kd_in);
  auto* kd_out = reinterpret_cast<unsigned long long*>(base + l.kd_out);
  auto* pos_in = reinterpret_cast<unsigned*>(base + l.pos_in);
  auto* pos_out = reinterpret_cast<unsigned*>(base + l.pos_out);
  auto* ks_in = reinterpret_cast<unsigned*>(base + l.ks_in);
  auto* ks_out = reinterpret_cast<unsigned*>(base + l.ks_out);
  auto* ps_out = reinterpret_cast<unsigned*>(base + l.ps_out);
  int* cnt = reinterpret_cast<int*>(base + l.cnt);
  float* dis = reinterpret_cast<float*>(base + l.dis);
  const int cb = cheb_col_bits(N);
  const bool weighted = w != nullptr && E > 0;
  if (!weighted && hipMemsetAsync(cnt, 0, (size_t)N * sizeof(int), st) != hipSuccess) {
    set_error("cheb_laplacian: clearing the degree counts failed");
    return TGMX_E_LAUNCH;
  }
  if (E > 0) {  // (a zero-length sort is not issued)
    hipLaunchKernelGGL(cheb_keys_kernel, dim3(cheb_grid(E, 256, 4096)), dim3(256), 0, st, src, dst, idx64, (long long)E, (long long)N, cb, kd_in,
                       pos_in, weighted ? ks_in : nullptr, cnt, skipped);
    TGMX_CHECK_LAUNCH("cheb_laplacian(keys)");
    size_t tb = l.temp_bytes;
    if (weighted) {
      int sb = 1;
      while ((1ll << sb) <= N) ++sb;  // the keys go up to N itself (the skipped edges)
      if (rocprim::radix_sort_pairs(base + l.temp, tb, (const unsigned*)ks_in, ks_out, (const unsigned*)pos_in, ps_out, (size_t)E, 0u, (unsigned)sb,
                                    st) != hipSuccess) {
        set_error("cheb_laplacian: radix sort (by source) failed");
        return TGMX_E_LAUNCH;
      }
    }
    tb = l.temp_bytes;
    if (rocprim::radix_sort_pairs(base + l.temp, tb, (const unsigned long long*)kd_in, kd_out, (const unsigned*)pos_in, pos_out, (size_t)E, 0u,
                                  (unsigned)(2 * cb + 1), st) != hipSuccess) {
      set_error("cheb_laplacian: radix sort (by destination) failed");
      return TGMX_E_LAUNCH;
    }
  }
  hipLaunchKernelGGL(cheb_degree_kernel, dim3(cheb_grid(N, kChebWaves, 4096)), dim3(kChebThreads), 0, st, weighted ? ks_out : nullptr, ps_out, w, cnt,
                     (long long)E, (long long)N, normalization, lambda_max, lambda_ptr, dis, diag);
  TGMX_CHECK_LAUNCH("cheb_laplacian(degree)");
  hipLaunchKernelGGL(cheb_rows_kernel, dim3(cheb_grid(E > N + 1 ? E : N + 1, 256, 4096)), dim3(256), 0, st, kd_out, pos_out, w, dis, (long long)E,
                     (long long)N, cb, normalization, lambda_max, lambda_ptr, indptr, cols, vals);
  TGMX_CHECK_LAUNCH("cheb_laplacian(rows)");
  return TGMX_OK;
}

extern "C" size_t tgmx_cheb_propagate_scratch_floats(int64_t nnz, int32_t C) {
  if (nnz <= kChebVeryLong || C <= 0) return 0;  // no row can be very long
  return (size_t)((nnz + kChebChunk - 1) / kChebChunk) * 2 * (size_t)C;
}

extern "C" int tgmx_cheb_propagate(const int32_t* indptr, const int32_t* cols, const float* vals, const float* diag, int64_t N, int32_t C,
                                   const float* t, int64_t ldt, const float* prev, int64_t ldp, float alpha, float beta, float* out, int64_t ldo,
                                   int64_t nnz, float* scratch, size_t scratch_floats, tgmx_stream_t stream) {
  TGMX_REQUIRE(N >= 0 && N < (1ll << 31) && C > 0 && ldt >= C && ldo >= C && (beta == 0.f || ldp >= C) && nnz >= 0 && nnz < (1ll << 31),
               "cheb_propagate: bad sizes N=%lld C=%d nnz=%lld", (long long)N, C, (long long)nnz);
  if (N == 0) return TGMX_OK;
  TGMX_REQUIRE(indptr && diag && t && out && (beta == 0.f || prev), "cheb_propagate: null pointer");
  // very long rows leave the first launch only when the caller brought the scratch for their chunk sums
  const size_t need = tgmx_cheb_propagate_scratch_floats(nnz, C);
  const bool chunks = need > 0 && scratch != nullptr;
  if (chunks && scratch_floats < need) {
    set_error("cheb_propagate: scratch too small (%zu floats, %zu needed)", scratch_floats, need);
    return TGMX_E_INVALID;
  }
  ChebProp a{indptr, cols, vals, diag, (long long)N, C, t, (long long)ldt, prev, (long long)ldp, alpha, beta, out, (long long)ldo,
             chunks ? kChebVeryLong : 0x7fffffff, chunks ? scratch : nullptr};
  auto vec_ok = [](const float* p, long long ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; };
  const bool vec = C % 4 == 0 && vec_ok(t, ldt) && vec_ok(out, ldo) && (beta == 0.f || vec_ok(prev, ldp)) && (!chunks || vec_ok(scratch, 4));
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((N + kChebWaves - 1) / kChebWaves)), block(kChebThreads);
  if (vec) hipLaunchKernelGGL(cheb_propagate_kernel<true>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(cheb_propagate_kernel<false>, grid, block, 0, st, a);
  TGMX_CHECK_LAUNCH("cheb_propagate");
  if (chunks) {
    const dim3 cgrid((unsigned)((nnz + kChebChunk - 1) / kChebChunk));
    if (vec) hipLaunchKernelGGL(cheb_chunk_kernel<true>, cgrid, block, 0, st, a);
    else hipLaunchKernelGGL(cheb_chunk_kernel<false>, cgrid, block, 0, st, a);
    TGMX_CHECK_LAUNCH("cheb_propagate(chunks)");
    if (vec) hipLaunchKernelGGL(cheb_join_kernel<true>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(cheb_join_kernel<false>, grid, block, 0, st, a);
    TGMX_CHECK_LAUNCH("cheb_propagate(join)");
  }
  return TGMX_OK;
}

extern "C" int tgmx_gclstm_forward(const tgmx_gclstm_fwd_t* a, tgmx_stream_t stream) {
  TGMX_REQUIRE(a, "gclstm_forward: null argument block");
  const int64_t N = a->N;
  const int C = a->C, K = a->K, in = a->in_ch;
  TGMX_REQUIRE(N > 0 && N < (1ll << 31) && C > 0 && K > 0 && in > 0 && a->E >= 0, "gclstm_forward: bad sizes");
  const long long width = (long long)in + (long long)K * C;
  TGMX_REQUIRE(width < (1ll << 31) && a->ldop >= width && a->ldw >= width, "gclstm_forward: operand narrower than in_ch + K C");
  TGMX_REQUIRE(a->x && a->W && a->b && a->H && a->Cprev && a->op && a->pre && a->H_out && a->C_out, "gclstm_forward: null pointer");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (K > 1 && (rc = tgmx_cheb_laplacian(a->src, a->dst, a->idx64, a->edge_w, a->E, N, a->normalization, a->lambda_max, a->lambda_ptr, a->indptr,
                                         a->cols, a->vals, a->diag, a->lap_ws, a->lap_ws_bytes, a->skipped, stream)))
    return rc;
  const long long fill = in + C + (a->ldop - width);
  hipLaunchKernelGGL(gclstm_operand_kernel, dim3(cheb_grid(N * fill, 256, 16384)), dim3(256), 0, st, a->x, in, a->H, C, (int)width, (long long)N,
                     a->op, (long long)a->ldop);
  TGMX_CHECK_LAUNCH("gclstm_forward(operand)");
  for (int k = 1; k < K; ++k) {  // Tx_1 = L_hat Tx_0;  Tx_k = 2 L_hat Tx_{k-1} - Tx_{k-2}
    float* tx = a->op + in + (long long)k * C;
    if ((rc = tgmx_cheb_propagate(a->indptr, a->cols, a->vals, a->diag, N, C, tx - C, a->ldop, k > 1 ? tx - 2 * C : nullptr, a->ldop,
                                  k > 1 ? 2.f : 1.f, k > 1 ? -1.f : 0.f, tx, a->ldop, a->E, a->prop_ws, a->prop_ws_floats, stream)))
      return rc;
  }
  if ((rc = tgmx_sgemm_nt(a->op, a->ldop, a->W, a->ldw, a->pre, 4 * C, N, 4 * C, (int32_t)width, a->b, 0, 1, 0, 0, 0, stream))) return rc;
  hipLaunchKernelGGL(gclstm_gates_kernel, dim3(cheb_grid(N * C, 256, 16384)), dim3(256), 0, st, a->pre, a->Cprev, C, (long long)N, a->H_out, a->C_out);
  TGMX_CHECK_LAUNCH("gclstm_forward(gates)");
  return TGMX_OK;
}
