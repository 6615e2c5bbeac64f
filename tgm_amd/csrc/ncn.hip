// NCNPredictor, the common-neighbour decoder of TNCN (the reference's tgm/nn/decoder/ncnpred.py), for gfx950: the symmetric adjacency of a
// batch's sampled subgraph as sorted rows, the per-pair row intersection with its gather-sum over x, and the inference forward as one call
// (the two Linear layers run on the exact-fp32 MFMA GEMM of csrc/dense.hip through tgmx_sgemm_nt_ep).
//
// Adjacency: the builder of edge_csr.h over the 2 E half-edges (a -> b) and (b -> a), keys only: the sorted keys ARE the adjacency (equal
// keys are interchangeable, so no edge position rides along).  Dropped: an edge with an endpoint outside [0, N).  The rows keep
// multiplicities as repeated entries; a row may be as long as 2 E.
//
// Pair kernel: one wave per pair.  The lanes take entries of the shorter row, 64 at a time; the first entry of every run of equal ids
// binary-searches the longer row (and its own run's end), the wave ballots the matches and visits them in ascending id, the lanes spread
// over the channels.  The order of the sum is fixed and there are no float atomics: two runs give the same bits.
#include "common.h"
#include "edge_csr.h"
#include "ncn_rows.h"

namespace tgmx {

constexpr int kNcnThreads = 256;
constexpr int kNcnWaves = kNcnThreads / kWave;
constexpr int kNcnChPerLane = 4;  // channels a lane accumulates per pass over the intersection: 256 channels a pass

// ---- adjacency ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ncn_keys_kernel(const void* __restrict__ ei, int is64, long long stride, long long E, long long N, int cb,
                                                       unsigned long long* __restrict__ keys) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long h = (long long)blockIdx.x * blockDim.x + threadIdx.x; h < 2 * E; h += step) {
    const long long e = h < E ? h : h - E;
    const long long a = ld_idx(ei, is64, e), b = ld_idx(ei, is64, stride + e);
    const bool ok = a >= 0 && a < N && b >= 0 && b < N;
    const long long row = h < E ? a : b, col = h < E ? b : a;
    keys[h] = key_of(ok, row, col, cb);
  }
}

struct AdjWorkspace {
  unsigned long long *k_in, *k_out;
  char* temp;
  size_t temp_bytes, total;
};
static int adj_carve(void* workspace, long long E, AdjWorkspace& w) {
  WorkspaceCarver c(workspace);
  const size_t n = (size_t)(E > 0 ? 2 * E : 1);
  w.k_in = c.take<unsigned long long>(n);
  w.k_out = c.take<unsigned long long>(n);
  w.temp_bytes = 0;
  if (rocprim::radix_sort_keys(nullptr, w.temp_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, n, 0u, 64u) != hipSuccess)
    return TGMX_E_LAUNCH;
  w.temp = c.take<char>(w.temp_bytes);
  w.total = c.total();
  return TGMX_OK;
}

// ---- the pairs ----------------------------------------------------------------------------------------------------------------------------
// last[side N + id] = the last position r at which id occurs on that side (the reference's mapping[rows] = arange(len(rows)) keeps the last
// write on the CPU); an integer max does not depend on the order of arrival
__global__ __launch_bounds__(256) void ncn_last_kernel(const void* __restrict__ tar, int is64, long long stride, long long B, long long N,
                                                       int32_t* __restrict__ last) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < 2 * B; t += step) {
    const int side = t >= B;
    const long long r = side ? t - B : t;
    const long long i = ld_idx(tar, is64, r), j = ld_idx(tar, is64, stride + r);
    // a pair with either target outside the node table gets a zero row: it marks nothing, on either side
    if (i >= 0 && i < N && j >= 0 && j < N) atomicMax(&last[side * N + (side ? j : i)], (int)r);
  }
}

int ncn_last_marks(const void* tar, int tar_is64, long long tar_stride, long long B, long long N, int32_t* last, hipStream_t st) {
  if (hipMemsetAsync(last, 0xff, (size_t)N * 2 * sizeof(int32_t), st) != hipSuccess) {  // -1: the id occurs nowhere
    set_error("ncn_cn_emb: clearing the last-occurrence marks failed");
    return TGMX_E_LAUNCH;
  }
  hipLaunchKernelGGL(ncn_last_kernel, dim3(grid_for(2 * B, 256, 4096)), dim3(256), 0, st, tar, tar_is64, tar_stride, B, N, last);
  TGMX_CHECK_LAUNCH("ncn_cn_emb(last)");
  return TGMX_OK;
}

struct CnArgs {
  const float* x;
  long long N;
  int C, k;
  const int32_t* indptr;
  const int32_t* cols;
  const void* tar;
  int tar_is64;
  long long tar_stride, B;
  const int64_t* last_update;  // NULL: no time decay
  const int64_t* edge_time;
  const int32_t* last;  // NULL: every row keeps its adjacency row
  float* xs;
  long long ldxs;
};

__global__ __launch_bounds__(kNcnThreads) void ncn_cn_kernel(CnArgs a) {
  const int lane = lane_id();
  const long long wave = (long long)blockIdx.x * kNcnWaves + threadIdx.x / kWave;
  const long long nwaves = (long long)gridDim.x * kNcnWaves;
  const int C = a.C;
  const float* __restrict__ x = a.x;
  const int32_t* __restrict__ cols = a.cols;
  for (long long r = wave; r < a.B; r += nwaves) {
    const long long ti = ld_idx(a.tar, a.tar_is64, r), tj = ld_idx(a.tar, a.tar_is64, a.tar_stride + r);
    float* __restrict__ o = a.xs + r * a.ldxs;
    if (ti < 0 || ti >= a.N || tj < 0 || tj >= a.N) {  // a target outside the node table is not dereferenced: a zero row
      for (long long c = lane; c < a.ldxs; c += kWave) o[c] = 0.f;
      continue;
    }
    const float* __restrict__ xi = x + ti * C;
    const float* __restrict__ xj = x + tj * C;
    for (int c = lane; c < C; c += kWave) o[c] = xi[c] * xj[c];
    for (long long c = (long long)a.k * C + lane; c < a.ldxs; c += kWave) o[c] = 0.f;
    // both sides' rows count only where this is the last occurrence of the target on its side
    const bool act = !a.last || (a.last[ti] == (int)r && a.last[a.N + tj] == (int)r);
    const bool decay = a.last_update != nullptr;
    const long long et = decay ? (long long)a.edge_time[r] : 0;
    const int ilo = a.indptr[ti], ihi = a.indptr[ti + 1], jlo = a.indptr[tj], jhi = a.indptr[tj + 1];
    float* __restrict__ cn = o + (a.k == 4 ? 3 * (long long)C : (long long)C);
    if (a.k == 4) {
      // (I_i o R_j o W) x and (R_i o I_j o W) x have one entry each: A[tj, ti] at column ti, A[ti, tj] at column tj (A is symmetric)
      const int m = act ? count_in(cols, ilo, ihi, tj) : 0;
      const float w0 = m ? (float)m * (decay ? decay_weight(a.last_update, et, ti) : 1.f) : 0.f;
      const float w1 = m ? (float)m * (decay ? decay_weight(a.last_update, et, tj) : 1.f) : 0.f;
      for (int c = lane; c < C; c += kWave) {
        o[C + c] = m ? w0 * xi[c] : 0.f;
        o[2 * (long long)C + c] = m ? w1 * xj[c] : 0.f;
      }
    }
    const bool i_short = ihi - ilo <= jhi - jlo;
    const int slo = i_short ? ilo : jlo, shi = i_short ? ihi : jhi, llo = i_short ? jlo : ilo, lhi = i_short ? jhi : ihi;
    for (int c0 = 0; c0 < C; c0 += kWave * kNcnChPerLane) {
      float acc[kNcnChPerLane];
#pragma unroll
      for (int q = 0; q < kNcnChPerLane; ++q) acc[q] = 0.f;
      if (act) {
        for (int p0 = slo; p0 < shi; p0 += kWave) {  // (the bounds are the wave's: every lane takes every trip)
          const int p = p0 + lane;
          const bool in = p < shi;
          const int n = in ? cols[p] : -1;
          const bool head = in && (p == slo || cols[p - 1] != n);  // one term per distinct id
          const int ml = head ? count_in(cols, llo, lhi, n) : 0;
          float w = 0.f;
          if (ml > 0) {
            const int ms = lower_bound_i32(cols, p, shi, (long long)n + 1) - p;
            w = (float)ms * (float)ml;
            if (decay) w *= decay_weight(a.last_update, et, n);
          }
          unsigned long long hits = __ballot(ml > 0);
          while (hits) {  // ascending lanes = ascending ids
            const int b = __ffsll((long long)hits) - 1;
            hits &= hits - 1;
            const int nn = __shfl(n, b);
            const float ww = __shfl(w, b);
            const float* __restrict__ xr = x + (long long)nn * C + c0;
#pragma unroll
            for (int q = 0; q < kNcnChPerLane; ++q) {
              const int c = lane + q * kWave;
              if (c0 + c < C) acc[q] = __fmaf_rn(ww, xr[c], acc[q]);
            }
          }
        }
      }
#pragma unroll
      for (int q = 0; q < kNcnChPerLane; ++q) {
        const int c = c0 + lane + q * kWave;
        if (c < C) cn[c] = acc[q];
      }
    }
  }
}

}  // namespace tgmx

using namespace tgmx;

extern "C" size_t tgmx_ncn_adj_workspace_bytes(int64_t E) {
  AdjWorkspace w;
  if (E < 0 || 2 * E >= (1ll << 31)) return 0;
  return adj_carve(nullptr, E, w) == TGMX_OK ? w.total : 0;
}

extern "C" int tgmx_ncn_adj_build(const void* edge_index, int32_t is64, int64_t row_stride, int64_t E, int64_t N, int32_t* indptr,
                                  int32_t* cols, void* workspace, size_t workspace_bytes, tgmx_stream_t stream) {
  TGMX_REQUIRE(E >= 0 && 2 * E < (1ll << 31) && N > 0 && N < (1ll << 31) && row_stride >= E, "ncn_adj_build: bad sizes E=%lld N=%lld row_stride=%lld",
               (long long)E, (long long)N, (long long)row_stride);
  TGMX_REQUIRE(indptr && (E == 0 || (edge_index && cols && workspace)), "ncn_adj_build: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int cb = col_bits(N);
  const long long n = 2 * E;
  const unsigned long long* sorted = nullptr;
  if (E > 0) {
    AdjWorkspace w;
    if (adj_carve(workspace, E, w) != TGMX_OK || workspace_bytes < w.total) {
      set_error("ncn_adj_build: workspace too small (%zu bytes)", workspace_bytes);
      return TGMX_E_INVALID;
    }
    hipLaunchKernelGGL(ncn_keys_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, st, edge_index, is64, (long long)row_stride, (long long)E,
                       (long long)N, cb, w.k_in);
    TGMX_CHECK_LAUNCH("ncn_adj_build(keys)");
    if (rocprim::radix_sort_keys(w.temp, w.temp_bytes, (const unsigned long long*)w.k_in, w.k_out, (size_t)n, 0u, (unsigned)(2 * cb + 1), st) !=
        hipSuccess) {
      set_error("ncn_adj_build: radix sort failed");
      return TGMX_E_LAUNCH;
    }
    sorted = w.k_out;
  }
  csr_rows_launch(sorted, n, (long long)N, cb, indptr, cols, NoEntryValue{}, st);
  TGMX_CHECK_LAUNCH("ncn_adj_build(rows)");
  return TGMX_OK;
}

extern "C" int tgmx_ncn_cn_emb(const float* x, int64_t N, int32_t C, int32_t k, const int32_t* indptr, const int32_t* cols, const void* tar,
                               int32_t tar_is64, int64_t tar_stride, int64_t B, const int64_t* last_update, const int64_t* edge_time,
                               int32_t* last, float* xs, int64_t ldxs, tgmx_stream_t stream) {
  TGMX_REQUIRE((k == 2 || k == 4) && C > 0 && N > 0 && N < (1ll << 31) && B >= 0 && B < (1ll << 31) && tar_stride >= B && ldxs >= (int64_t)k * C,
               "ncn_cn_emb: bad sizes k=%d (2 or 4) C=%d N=%lld B=%lld ldxs=%lld", k, C, (long long)N, (long long)B, (long long)ldxs);
  if (B == 0) return TGMX_OK;
  TGMX_REQUIRE(x && indptr && cols && tar && xs, "ncn_cn_emb: null pointer");
  TGMX_REQUIRE((last_update == nullptr) == (edge_time == nullptr), "ncn_cn_emb: time decay needs last_update and edge_time");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (last && (rc = ncn_last_marks(tar, tar_is64, (long long)tar_stride, (long long)B, (long long)N, last, st))) return rc;
  CnArgs a{x, (long long)N, C, k, indptr, cols, tar, tar_is64, (long long)tar_stride, (long long)B, last_update, edge_time, last, xs, (long long)ldxs};
  hipLaunchKernelGGL(ncn_cn_kernel, dim3(grid_for(B, kNcnWaves, 16384)), dim3(kNcnThreads), 0, st, a);
  TGMX_CHECK_LAUNCH("ncn_cn_emb");
  return TGMX_OK;
}

extern "C" int tgmx_ncn_forward(const tgmx_ncn_fwd_t* a, tgmx_stream_t stream) {
  TGMX_REQUIRE(a && a->H > 0 && a->out_ch > 0 && a->B >= 0 && a->C > 0, "ncn_forward: bad argument block");
  TGMX_REQUIRE(a->ldxs % 4 == 0 && a->ldh % 4 == 0 && a->ldh >= a->H, "ncn_forward: leading dimensions must be multiples of 4");
  int rc;
  if (!a->have_adj &&
      (rc = tgmx_ncn_adj_build(a->edge_index, a->ei_is64, a->ei_stride, a->E, a->N, a->indptr, a->cols, a->adj_ws, a->adj_ws_bytes, stream)))
    return rc;
  if (a->B == 0) return TGMX_OK;
  if ((rc = tgmx_ncn_cn_emb(a->x, a->N, a->C, a->k, a->indptr, a->cols, a->tar, a->tar_is64, a->tar_stride, a->B, a->decay ? a->last_update : nullptr,
                            a->decay ? a->edge_time : nullptr, a->dup_all ? nullptr : a->last, a->xs, a->ldxs, stream)))
    return rc;
  TGMX_REQUIRE(a->w1 && a->b1 && a->w2 && a->b2 && a->h && a->out, "ncn_forward: null pointer");
  const int K = a->k * a->C;
  // (the reference's xs.relu() discards its result: negative entries reach the first Linear)
  if ((rc = tgmx_sgemm_nt_ep(a->xs, a->ldxs, a->w1, K, a->h, a->ldh, a->B, a->H, K, a->b1, 1, nullptr, 0, stream))) return rc;
  return tgmx_sgemm_nt_ep(a->h, a->ldh, a->w2, a->H, a->out, a->out_ch, a->B, a->out_ch, a->H, a->b2, 0, nullptr, 0, stream);
}
