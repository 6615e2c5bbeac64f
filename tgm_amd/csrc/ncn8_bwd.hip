// Training of NCNPredictor at k = 8 (ncn8.hip's forward), for gfx950: the gradient of x through the eight blocks of xs, and the whole backward
// as ONE call.  With g_b[r] the C-wide block b of dxs[r] = (dpre W1)[r] and T[8 r + b, n] the coefficient the forward applied to x[n] in block
// b of pair r (the count times W[r, n] on blocks 1-6, the bare count on block 7, row 8 r all zero):
//
//   dx[n] = sum over r in range, i_r = n of g_0[r] * x[j_r]  +  sum over r in range, j_r = n of g_0[r] * x[i_r]  +  (T^T dxs)[n]
//
// where dxs is read as an [8 B, C] matrix (its rows are contiguous: lddxs = 8 C), which lines up with T row for row.
//
// 1. ncn8_dx_pairs_kernel -- node-centred: a wave owns a node and adds the first two sums in ascending r through ncn_bwd.hip's two inverted
//    indexes of the pairs, one fmaf per term, 256 channels in registers, and STORES every row of dx (zeros included).
// 2. ncn8_coef_kernel<kLds> -- pair-centred, because one two-hop walk of the two targets gives the coefficients of EVERY n: a workgroup per
//    pair of a slab of P pairs builds the forward's five int32 count rows (ncn8_rows.h: the same walk, the same storage -- LDS up to
//    kNcn8LdsMaxN ids, a 5 N int32 region per resident workgroup above, cleared by walking again), K3[i, i], K3[j, j], u, then takes the ids
//    256 at a time, a thread each, and stores the seven coefficients of n, each count times W in float64 rounded once (W the forward's,
//    applied only where the count is non-zero), into rows 8 s + 1 .. 8 s + 7 of the slab -- coalesced along n.  The slab's zeros are STORED:
//    every workgroup writes all 8 ldT floats of its pair (row 8 s, the pad columns, the rows of an inactive or out-of-range pair), so no
//    memset of the slab precedes it and every element is defined before the product reads it.
// 3. tgmx_sgemm_tn (exact-fp32 MFMA, fixed two-stage reduction) adds T_slab^T dxs_slab onto what step 1 stored; slabs in ascending pair order.
//
// No float atomics; the count rows are integer atomics.  The order of dx's sum is fixed by (sizes, slab size): two runs give the same bits.
// DIFFERENT slab sizes group the sum differently and agree only within rounding (a few float32 ulps of the largest term), not bit for bit.
// Nothing [B, N] outlives the call: the slab is the only dense coefficient storage, 32 ldT bytes per pair.
#include "ncn8_rows.h"

namespace tgmx {

// The slab budget: P = min(B, max(1, kNcn8BwdSlabBytes / (32 ldT))) pairs per slab.  A larger budget means fewer slabs -- fewer coefficient
// launches and fewer, taller GEMMs (each GEMM costs two launches and re-reads dx) -- against more transient memory; a smaller one the
// reverse.  256 MiB holds the example's whole batch (200 pairs, ~1000 ids: 6.5 MB) many times over and still covers 1000 pairs at 8000 ids in
// one slab.  The value has NOT been tuned by measurement.
constexpr long long kNcn8BwdSlabBytes = 256ll << 20;
constexpr int kNcn8BwdChPerLane = 4;  // channels a lane of the pair-term kernel accumulates per pass: 256 a pass

struct Coef8Args {
  long long N;
  const int32_t* indptr;
  const int32_t* cols;
  const void* tar;
  int tar_is64;
  long long tar_stride, first, P;  // the slab's pairs: [first, first + P)
  const int64_t* last_update;      // NULL: no time decay
  const int64_t* edge_time;
  const int32_t* last;  // NULL: every in-range pair is active
  float* T;             // [8 P, ldT]
  long long ldT;
  int32_t* ws;  // the workspace form's regions
  long long region;
};

template <bool kLds>
__global__ __launch_bounds__(kNcn8Threads) void ncn8_coef_kernel(Coef8Args a) {
  using Rw = Rows<kLds>;
  extern __shared__ int32_t s_rows[];
  __shared__ long long s_k3[kNcn8Waves][2];
  const int tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
  const long long N = a.N, ldT = a.ldT;
  const int32_t* __restrict__ cols = a.cols;
  int32_t* rows = kLds ? s_rows : a.ws + (long long)blockIdx.x * a.region;
  int32_t *Ri = rows, *Rj = rows + N, *Si = rows + 2 * N, *Sj = rows + 3 * N, *sp = rows + 4 * N;
  for (long long s = blockIdx.x; s < a.P; s += gridDim.x) {  // (s is the workgroup's: every barrier below is reached by all)
    const long long r = a.first + s;
    const long long ti = ld_idx(a.tar, a.tar_is64, r), tj = ld_idx(a.tar, a.tar_is64, a.tar_stride + r);
    float* __restrict__ Ts = a.T + 8 * s * ldT;
    // a target outside the node table is not dereferenced; a pair that is not the last occurrence of both targets has zero blocks
    const bool in = ti >= 0 && ti < N && tj >= 0 && tj < N;
    const bool act = in && (!a.last || (a.last[ti] == (int)r && a.last[N + tj] == (int)r));
    if (!act) {
      for (long long c = tid; c < 8 * ldT; c += kNcn8Threads) Ts[c] = 0.f;
      continue;
    }
    const bool decay = a.last_update != nullptr;
    const long long et = decay ? (long long)a.edge_time[r] : 0;
    const int ilo = a.indptr[ti], ihi = a.indptr[ti + 1], jlo = a.indptr[tj], jhi = a.indptr[tj + 1];

    // ---- the count rows, as the forward builds them ----
    if (kLds) {
      for (long long t = tid; t < kNcn8Rows * N; t += kNcn8Threads) s_rows[t] = 0;
      __syncthreads();
    }
    ncn8_walk<kLds, false>(a.indptr, cols, ilo, ihi, jlo, jhi, Ri, Si, sp);
    ncn8_walk<kLds, false>(a.indptr, cols, jlo, jhi, 0, 0, Rj, Sj, nullptr);
    Rw::sync();

    // ---- K3[i, i], K3[j, j], u ----
    long long k3i = ncn8_k3_part<kLds>(cols, ilo, ihi, Si), k3j = ncn8_k3_part<kLds>(cols, jlo, jhi, Sj);
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      k3i += __shfl_down(k3i, off);
      k3j += __shfl_down(k3j, off);
    }
    if (lane == 0) s_k3[wave][0] = k3i, s_k3[wave][1] = k3j;
    __syncthreads();
    k3i = k3j = 0;
#pragma unroll
    for (int w = 0; w < kNcn8Waves; ++w) k3i += s_k3[w][0], k3j += s_k3[w][1];
    const long long mij = count_in(cols, ilo, ihi, tj);  // A[i, j] = A[j, i]
    const long long u = -mij;

    // ---- the seven coefficients of every id, a thread each; the pad columns [N, ldT) and row 8 s get their zeros here ----
    for (long long n = tid; n < ldT; n += kNcn8Threads) {
      float v[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (n < N) {
        const long long ri = Rw::ld(Ri + n), rj = Rw::ld(Rj + n), si = Rw::ld(Si + n), sj = Rw::ld(Sj + n), cs = Rw::ld(sp + n);
        long long cf[6] = {n == ti ? mij : 0, n == tj ? mij : 0, ri * rj, 0, 0, 0};  // c01, c10, c11, c12, c21, c22
        if (n != ti && n != tj) {  // the column masks of c12, c21, c22
          cf[3] = ri * sj + ri * ri * u;
          cf[4] = si * rj + rj * rj * u;
          cf[5] = si * sj + ((ri > 0 ? k3i : 0) + (rj > 0 ? k3j : 0) - cf[2]) * u + cs;
          if (cf[5] < 0) cf[5] = 0;
        }
        // W is applied only where a count is non-zero, as in the forward (an infinite weight leaves the zeros alone)
        const bool weighted = (cf[0] | cf[1] | cf[2] | cf[3] | cf[4] | cf[5]) != 0;
        const double w = decay && weighted ? decay_weight_f64(a.last_update, et, n) : 1.;
#pragma unroll
        for (int q = 0; q < 6; ++q) v[q] = cf[q] != 0 ? (float)((double)(float)cf[q] * w) : 0.f;  // (the forward converts the count first)
        v[6] = (float)cs;  // special_2_2 carries no decay and no column mask
      }
      Ts[n] = 0.f;
#pragma unroll
      for (int q = 0; q < 7; ++q) Ts[(q + 1) * ldT + n] = v[q];
    }
    Rw::sync();  // every row is read before the next pair (or the walk below) clears it

    if (!kLds) {  // leave the region zeroed for the next pair: the same walks, storing zeros
      ncn8_walk<kLds, true>(a.indptr, cols, ilo, ihi, jlo, jhi, Ri, Si, sp);
      ncn8_walk<kLds, true>(a.indptr, cols, jlo, jhi, 0, 0, Rj, Sj, nullptr);
      Rw::sync();
    }
  }
}

struct DxPairs8Args {
  const float* x;
  long long N;
  int C;
  const void* tar;
  int tar_is64;
  long long tar_stride;
  const float* dxs;
  long long lddxs;
  const int32_t* bt_ptr;  // [2 N + 1]: the pairs by tar_i (rows [0, N)) and by tar_j (rows [N, 2 N))
  const int32_t* bt_r;
  float* dx;
};

// a wave per node: the pairs that hold it as tar_i, then as tar_j, each list in ascending r (a pair with i = j is in both); every row is stored
__global__ __launch_bounds__(kNcn8Threads) void ncn8_dx_pairs_kernel(DxPairs8Args a) {
  const int lane = lane_id();
  const long long nwaves = (long long)gridDim.x * kNcn8Waves;
  for (long long n = (long long)blockIdx.x * kNcn8Waves + threadIdx.x / kWave; n < a.N; n += nwaves) {
    for (int c0 = 0; c0 < a.C; c0 += kWave * kNcn8BwdChPerLane) {
      float acc[kNcn8BwdChPerLane] = {0.f, 0.f, 0.f, 0.f};
      for (int side = 0; side < 2; ++side) {
        const int lo = a.bt_ptr[side * a.N + n], hi = a.bt_ptr[side * a.N + n + 1];
        for (int q = lo; q < hi; ++q) {  // (q, r and the other target are the wave's)
          const long long r = a.bt_r[q];
          const long long other = ld_idx(a.tar, a.tar_is64, side ? r : a.tar_stride + r);  // inside [0, N): the index left the others out
          const float* __restrict__ g0 = a.dxs + r * a.lddxs + c0;
          const float* __restrict__ xo = a.x + other * a.C + c0;
#pragma unroll
          for (int u = 0; u < kNcn8BwdChPerLane; ++u) {
            const int c = lane + u * kWave;
            if (c0 + c < a.C) acc[u] = __fmaf_rn(g0[c], xo[c], acc[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kNcn8BwdChPerLane; ++u) {
        const int c = c0 + lane + u * kWave;
        if (c < a.C) a.dx[n * a.C + c] = acc[u];
      }
    }
  }
}

static std::atomic<bool> s_coef_optin[kNcn8MaxDevices];

static bool ncn8_bwd_sizes_ok(long long N, long long B, int C) {
  return C > 0 && N > 0 && 2 * N < (1ll << 31) && B >= 0 && 2 * B < (1ll << 31) && 8ll * C < (1ll << 31);
}
static long long ncn8_ldT(long long N) { return (N + 63) & ~63ll; }
static long long ncn8_bwd_slab(long long N, long long B, long long slab_pairs) {
  long long P = slab_pairs > 0 ? slab_pairs : kNcn8BwdSlabBytes / (32 * ncn8_ldT(N));
  if (P < 1) P = 1;
  return P < B ? P : (B > 0 ? B : 1);
}
static bool ncn8_rows_in_ws(long long N, int force_workspace) { return N > kNcn8LdsMaxN || force_workspace; }

// the slab rows of the pairs [a.first, a.first + a.P); rows: region * groups(P) int32 of workspace where the count rows do not live in LDS,
// zeroed here when `clear` (every pair clears its region behind it, so ONE clearing serves all the slabs of a tgmx_ncn8_dx call)
static int ncn8_coef_launch(Coef8Args a, int force_workspace, int32_t* rows, bool clear, hipStream_t st) {
  if (!ncn8_rows_in_ws(a.N, force_workspace)) {
    if (!ncn8_lds_optin(reinterpret_cast<const void*>(ncn8_coef_kernel<true>), s_coef_optin, "ncn8_coef")) return TGMX_E_LAUNCH;
    const size_t lds = (size_t)kNcn8Rows * (size_t)a.N * sizeof(int32_t);
    hipLaunchKernelGGL(ncn8_coef_kernel<true>, dim3(grid_for(a.P, 1, 16384)), dim3(kNcn8Threads), lds, st, a);
    TGMX_CHECK_LAUNCH("ncn8_coef");
    return TGMX_OK;
  }
  const long long groups = ncn8_groups(a.P);
  a.region = (long long)ncn8_region_ints(a.N);
  a.ws = rows;
  if (clear && hipMemsetAsync(rows, 0, (size_t)a.region * (size_t)groups * sizeof(int32_t), st) != hipSuccess) {
    set_error("ncn8_coef: clearing the workspace failed");
    return TGMX_E_LAUNCH;
  }
  hipLaunchKernelGGL(ncn8_coef_kernel<false>, dim3((unsigned)groups), dim3(kNcn8Threads), 0, st, a);
  TGMX_CHECK_LAUNCH("ncn8_coef(workspace)");
  return TGMX_OK;
}

static int ncn8_dx_pairs_launch(const DxPairs8Args& a, hipStream_t st) {
  hipLaunchKernelGGL(ncn8_dx_pairs_kernel, dim3(grid_for(a.N, kNcn8Waves, 16384)), dim3(kNcn8Threads), 0, st, a);
  TGMX_CHECK_LAUNCH("ncn8_dx_pairs");
  return TGMX_OK;
}

struct Dx8Workspace {
  NcnPairIndex bt;
  float *T, *part;
  int32_t* rows;
  size_t total;
};
static int ncn8_dx_carve(void* workspace, long long N, long long B, int C, long long P, int force_workspace, Dx8Workspace& w) {
  WorkspaceCarver c(workspace);
  if (ncn_pair_index_carve(c, N, B, w.bt) != TGMX_OK) return TGMX_E_LAUNCH;
  w.T = c.take<float>((size_t)(8 * P) * (size_t)ncn8_ldT(N));
  w.part = c.take<float>(tgmx_sgemm_tn_workspace_bytes(8 * P, (int32_t)N, C, 1) / sizeof(float));
  w.rows = c.take<int32_t>(ncn8_rows_in_ws(N, force_workspace) ? ncn8_region_ints(N) * (size_t)ncn8_groups(P) : 0);
  w.total = c.total();
  return TGMX_OK;
}

}  // namespace tgmx

using namespace tgmx;

extern "C" int64_t tgmx_ncn8_backward_slab_pairs(int64_t N, int64_t B, int64_t slab_pairs) {
  return N > 0 && B >= 0 ? ncn8_bwd_slab(N, B, slab_pairs) : 0;
}

extern "C" int tgmx_ncn8_coef(int64_t N, const int32_t* indptr, const int32_t* cols, const void* tar, int32_t tar_is64, int64_t tar_stride, int64_t B,
                              const int64_t* last_update, const int64_t* edge_time, const int32_t* last, int64_t first, int64_t P, float* T,
                              int64_t ldT, void* workspace, size_t workspace_bytes, int32_t force_workspace, tgmx_stream_t stream) {
  TGMX_REQUIRE(ncn8_bwd_sizes_ok(N, B, 1) && tar_stride >= B && first >= 0 && P >= 0 && first + P <= B && ldT >= N && ldT % 64 == 0,
               "ncn8_coef: bad sizes N=%lld B=%lld first=%lld P=%lld ldT=%lld (a multiple of 64, >= N)", (long long)N, (long long)B, (long long)first,
               (long long)P, (long long)ldT);
  if (P == 0) return TGMX_OK;
  TGMX_REQUIRE(indptr && cols && tar && T, "ncn8_coef: null pointer");
  TGMX_REQUIRE((last_update == nullptr) == (edge_time == nullptr), "ncn8_coef: time decay needs last_update and edge_time");
  int32_t* rows = nullptr;
  if (ncn8_rows_in_ws(N, force_workspace)) {
    WorkspaceCarver c(workspace);
    rows = c.take<int32_t>(ncn8_region_ints(N) * (size_t)ncn8_groups(P));
    if (!workspace || workspace_bytes < c.total()) {
      set_error("ncn8_coef: workspace too small (%zu bytes, %zu needed)", workspace_bytes, c.total());
      return TGMX_E_INVALID;
    }
  }
  const Coef8Args a{(long long)N, indptr, cols, tar, tar_is64 ? 1 : 0, (long long)tar_stride, (long long)first, (long long)P, last_update, edge_time, last,
                    T, (long long)ldT, nullptr, 0};
  return ncn8_coef_launch(a, force_workspace, rows, true, (hipStream_t)stream);
}

extern "C" size_t tgmx_ncn8_dx_pairs_workspace_bytes(int64_t N, int64_t B) {
  if (!ncn8_bwd_sizes_ok(N, B, 1)) return 0;
  WorkspaceCarver c(nullptr);
  NcnPairIndex bt;
  return ncn_pair_index_carve(c, N, B, bt) == TGMX_OK ? c.total() : 0;
}

extern "C" int tgmx_ncn8_dx_pairs(const float* x, int64_t N, int32_t C, const void* tar, int32_t tar_is64, int64_t tar_stride, int64_t B,
                                  const float* dxs, int64_t lddxs, float* dx, void* workspace, size_t workspace_bytes, tgmx_stream_t stream) {
  TGMX_REQUIRE(ncn8_bwd_sizes_ok(N, B, C) && tar_stride >= B && lddxs >= C, "ncn8_dx_pairs: bad sizes C=%d N=%lld B=%lld lddxs=%lld", C, (long long)N,
               (long long)B, (long long)lddxs);
  TGMX_REQUIRE(dx, "ncn8_dx_pairs: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {  // no pair: every row is zero
    if (hipMemsetAsync(dx, 0, (size_t)N * C * sizeof(float), st) != hipSuccess) {
      set_error("ncn8_dx_pairs: clearing dx failed");
      return TGMX_E_LAUNCH;
    }
    return TGMX_OK;
  }
  TGMX_REQUIRE(x && tar && dxs && workspace, "ncn8_dx_pairs: null pointer");
  WorkspaceCarver c(workspace);
  NcnPairIndex bt;
  if (ncn_pair_index_carve(c, N, B, bt) != TGMX_OK || workspace_bytes < c.total()) {
    set_error("ncn8_dx_pairs: workspace too small (%zu bytes)", workspace_bytes);
    return TGMX_E_INVALID;
  }
  int rc;
  if ((rc = ncn_pair_index_build(tar, tar_is64, (long long)tar_stride, (long long)B, (long long)N, bt, "ncn8_dx_pairs", st))) return rc;
  return ncn8_dx_pairs_launch(DxPairs8Args{x, (long long)N, C, tar, tar_is64 ? 1 : 0, (long long)tar_stride, dxs, (long long)lddxs, bt.ptr, bt.r, dx}, st);
}

extern "C" size_t tgmx_ncn8_dx_workspace_bytes(int64_t N, int64_t B, int32_t C, int64_t slab_pairs, int32_t force_workspace) {
  if (!ncn8_bwd_sizes_ok(N, B, C) || slab_pairs < 0) return 0;
  Dx8Workspace w;
  return ncn8_dx_carve(nullptr, N, B, C, ncn8_bwd_slab(N, B, slab_pairs), force_workspace, w) == TGMX_OK ? w.total : 0;
}

extern "C" int tgmx_ncn8_dx(const float* x, int64_t N, int32_t C, const int32_t* indptr, const int32_t* cols, const void* tar, int32_t tar_is64,
                            int64_t tar_stride, int64_t B, const int64_t* last_update, const int64_t* edge_time, const int32_t* last, const float* dxs,
                            int64_t lddxs, float* dx, int64_t slab_pairs, void* workspace, size_t workspace_bytes, int32_t force_workspace,
                            tgmx_stream_t stream) {
  TGMX_REQUIRE(ncn8_bwd_sizes_ok(N, B, C) && tar_stride >= B && slab_pairs >= 0, "ncn8_dx: bad sizes C=%d N=%lld B=%lld slab_pairs=%lld", C, (long long)N,
               (long long)B, (long long)slab_pairs);
  TGMX_REQUIRE(lddxs == 8ll * C, "ncn8_dx: dxs must be contiguous (lddxs = 8 C = %lld, got %lld): it is read as an [8 B, C] matrix", 8ll * C, (long long)lddxs);
  TGMX_REQUIRE(dx && indptr, "ncn8_dx: null pointer");
  TGMX_REQUIRE((last_update == nullptr) == (edge_time == nullptr), "ncn8_dx: time decay needs last_update and edge_time");
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {  // no pair: every row is zero
    if (hipMemsetAsync(dx, 0, (size_t)N * C * sizeof(float), st) != hipSuccess) {
      set_error("ncn8_dx: clearing dx failed");
      return TGMX_E_LAUNCH;
    }
    return TGMX_OK;
  }
  TGMX_REQUIRE(x && cols && tar && dxs && workspace, "ncn8_dx: null pointer");
  const long long P = ncn8_bwd_slab(N, B, slab_pairs), ldT = ncn8_ldT(N);
  Dx8Workspace w;
  if (ncn8_dx_carve(workspace, N, B, C, P, force_workspace, w) != TGMX_OK || workspace_bytes < w.total) {
    set_error("ncn8_dx: workspace too small (%zu bytes)", workspace_bytes);
    return TGMX_E_INVALID;
  }
  int rc;
  if ((rc = ncn_pair_index_build(tar, tar_is64, (long long)tar_stride, (long long)B, (long long)N, w.bt, "ncn8_dx", st))) return rc;
  if ((rc = ncn8_dx_pairs_launch(DxPairs8Args{x, (long long)N, C, tar, tar_is64 ? 1 : 0, (long long)tar_stride, dxs, (long long)lddxs, w.bt.ptr, w.bt.r, dx},
                                 st)))
    return rc;
  for (long long first = 0; first < B; first += P) {  // ascending pair order: the order of dx's sum is fixed by (sizes, P)
    const long long p = B - first < P ? B - first : P;
    const Coef8Args a{(long long)N, indptr, cols, tar, tar_is64 ? 1 : 0, (long long)tar_stride, first, p, last_update, edge_time, last, w.T, ldT, nullptr, 0};
    if ((rc = ncn8_coef_launch(a, force_workspace, w.rows, first == 0, st))) return rc;  // (the first slab is the largest: its regions cover the rest)
    if ((rc = tgmx_sgemm_tn(w.T, ldT, dxs + 8ll * C * first, C, dx, C, 8 * p, (int32_t)N, C, 1, 0, 0, 0, 1, w.part, stream))) return rc;
  }
  return TGMX_OK;
}

// ---- the whole backward ---------------------------------------------------------------------------------------------------------------------
static int ncn8_bwd_check(const tgmx_ncn_bwd_t* t, int64_t slab_pairs, const char* who) {
  TGMX_REQUIRE(t, "%s: null argument block", who);
  const tgmx_ncn_fwd_t& a = t->fwd;
  TGMX_REQUIRE(a.k == 8 && ncn8_bwd_sizes_ok(a.N, a.B, a.C) && slab_pairs >= 0 && a.E >= 0 && 2 * a.E < (1ll << 31) && a.H > 0 && a.out_ch > 0 &&
                   a.ldxs >= 8ll * a.C && a.ldh >= a.H && a.tar_stride >= a.B,
               "%s: bad sizes k=%d (must be 8) C=%d H=%d out=%d N=%lld E=%lld B=%lld slab_pairs=%lld", who, a.k, a.C, a.H, a.out_ch, (long long)a.N,
               (long long)a.E, (long long)a.B, (long long)slab_pairs);
  TGMX_REQUIRE(a.H <= 8192, "%s: hidden_dim %d is more than the 8192 the k = 8 forward takes", who, a.H);
  return TGMX_OK;
}

// One walk over the backward; dry: only the workspace is laid out (*need = its bytes), nothing is launched
static int ncn8_backward_pass(const tgmx_ncn_bwd_t* t, int64_t slab_pairs, bool dry, size_t* need, tgmx_stream_t stream) {
  const tgmx_ncn_fwd_t& a = t->fwd;
  int rc;
  WorkspaceCarver ws(dry ? nullptr : t->workspace);
  float* dxs = nullptr;
  if ((rc = ncn_mlp_backward(t, ws, dry, &dxs, stream))) return rc;
  if (t->d_x) {
    const size_t bytes = tgmx_ncn8_dx_workspace_bytes(a.N, a.B, a.C, slab_pairs, 0);
    if (bytes == 0) return TGMX_E_INVALID;
    char* dws = ws.take<char>(bytes);
    if (!dry && (rc = tgmx_ncn8_dx(a.x, a.N, a.C, a.indptr, a.cols, a.tar, a.tar_is64, a.tar_stride, a.B, a.decay ? a.last_update : nullptr,
                                   a.decay ? a.edge_time : nullptr, a.dup_all ? nullptr : a.last, dxs, 8ll * a.C, t->d_x, slab_pairs, dws, bytes, 0,
                                   stream)))
      return rc;
  }
  *need = ws.total();
  return TGMX_OK;
}

extern "C" size_t tgmx_ncn8_backward_workspace_bytes(const tgmx_ncn_bwd_t* t, int64_t slab_pairs) {
  size_t need = 0;
  if (ncn8_bwd_check(t, slab_pairs, "ncn8_backward_workspace_bytes") != TGMX_OK) return 0;
  return ncn8_backward_pass(t, slab_pairs, true, &need, nullptr) == TGMX_OK ? need : 0;
}

extern "C" int tgmx_ncn8_backward(const tgmx_ncn_bwd_t* t, int64_t slab_pairs, tgmx_stream_t stream) {
  int rc;
  if ((rc = ncn8_bwd_check(t, slab_pairs, "ncn8_backward"))) return rc;
  const tgmx_ncn_fwd_t& a = t->fwd;
  if (a.B == 0) return ncn_backward_empty(t, "ncn8_backward", stream);  // no pair: every gradient asked for is zero
  TGMX_REQUIRE(t->dout && t->lddout >= a.out_ch, "ncn8_backward: no upstream gradient");
  TGMX_REQUIRE(a.x && a.tar && a.w1 && a.w2 && a.xs && a.h && a.indptr && a.cols && (a.dup_all || a.last) &&
                   (!a.decay || (a.last_update && a.edge_time)),
               "ncn8_backward: null pointer");
  size_t need = 0;
  if ((rc = ncn8_backward_pass(t, slab_pairs, true, &need, nullptr))) return rc;
  TGMX_REQUIRE(t->workspace && t->workspace_bytes >= need, "ncn8_backward: workspace too small (%zu bytes, %zu needed)", t->workspace_bytes, need);
  return ncn8_backward_pass(t, slab_pairs, false, &need, stream);
}
