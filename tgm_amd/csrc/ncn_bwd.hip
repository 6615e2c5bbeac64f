// Training of NCNPredictor (ncn.hip's forward), for gfx950: the backward of the common-neighbour stage, and the whole backward as ONE call.
//
// dx is node-centred and reads the adjacency the forward built.  With g0 .. g3 the C-wide column blocks of dxs[r], node n receives
//   (1) from every in-range pair r with tar_i[r] = n:  g0[r] * x[tar_j[r]]   (+ k = 4, r active, m = A[i, j] > 0:  m W[r, i] g1[r])
//   (2) from every in-range pair r with tar_j[r] = n:  g0[r] * x[tar_i[r]]   (+ k = 4, r active, m > 0:            m W[r, j] g2[r])
//   (3) from every active pair r with A[n, i_r] > 0 and A[n, j_r] > 0:       A[n, i_r] A[n, j_r] W[r, n] g_cn[r]
// A is symmetric, so the pairs of (3) have their tar_i among the distinct ids of row n: two inverted indexes of the pairs, by tar_i and by
// tar_j (edge_csr.h's sorted keys ((side N + target) << cb | r), ONE radix sort of 2 B keys), are all the backward adds to the forward's rows.
//
// A wave owns a node and keeps 256 channels of its row in registers, stored once.  It walks (1) and (2) in ascending r, then the distinct
// ids a of row n in ascending order, 64 entries at a time (the first entry of a run is its head, the run's length is A[n, a]); the lanes
// take the pairs of a head's list 64 at a time, each searches tar_j[r] in row n (count_in), the wave ballots the hits and adds them in
// ascending r.  So the sum of a node is ordered by (term, a, r): fixed by the inputs, no float atomics, two runs give the same bits.
//
// A row of more than kNcnBwdLongRow entries (a hub: the row may hold all 2 E) leaves term (3) to two more launches, spmm.h's hub treatment:
// the ENTRY array is cut into chunks of kNcnBwdChunk, a wave per chunk sums the heads its chunk holds of the (at most two: the threshold is
// no shorter than a chunk) long rows it meets, and a join adds a row's chunk sums in ascending chunk order onto its terms (1) and (2).  The
// two launches are issued whenever 2 E exceeds the threshold: the host reads nothing back.
//
// Chain lengths (tests/ncn_bwd_restate.py counts them from here): a node's sum has one rounding per term, the k = 4 extra terms included;
// a long row's adds (terms of (1) and (2)) + (terms of a chunk) + (its chunks) at most.
#include "common.h"
#include "edge_csr.h"
#include "ncn_rows.h"

namespace tgmx {

constexpr int kNcnBwdThreads = 256;
constexpr int kNcnBwdWaves = kNcnBwdThreads / kWave;
constexpr int kNcnBwdChPerLane = 4;   // channels a lane accumulates per pass: 256 channels a pass, as in the forward
constexpr int kNcnBwdChunk = 256;     // entries of the adjacency one wave of the chunk launch covers
constexpr int kNcnBwdLongRow = 512;   // rows longer than this go through the chunk launches (>= kNcnBwdChunk: a chunk meets at most two)
constexpr int kNcnBwdMaxTail = 16;    // decoder.hip's kDecMaxTail

struct DxArgs {
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
  const int32_t* last;  // NULL: every in-range pair is active
  const float* dxs;
  long long lddxs;
  const int32_t* bt_ptr;  // [2 N + 1]: the pairs by tar_i (rows [0, N)) and by tar_j (rows [N, 2 N))
  const int32_t* bt_r;    // the pairs' positions, ascending within a row
  float* dx;
  int long_row;    // rows longer than this are left to the chunk launches
  float* scratch;  // [chunks, 2, C]
};

// key t < B: ((tar_i[t]) << cb | t);  key B + t: ((N + tar_j[t]) << cb | t).  A pair with a target outside [0, N) is in neither list.
__global__ __launch_bounds__(256) void ncn_bwd_keys_kernel(const void* __restrict__ tar, int is64, long long stride, long long B, long long N, int cb,
                                                           unsigned long long* __restrict__ keys) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < 2 * B; t += step) {
    const long long r = t < B ? t : t - B;
    const long long i = ld_idx(tar, is64, r), j = ld_idx(tar, is64, stride + r);
    const bool ok = i >= 0 && i < N && j >= 0 && j < N;
    keys[t] = key_of(ok, t < B ? i : N + j, r, cb);
  }
}

// terms (1) (side 0) or (2) (side 1) of node n, channels [c0, c0 + 256): the pairs in ascending r
__device__ __forceinline__ void ncn_bwd_pair_terms(const DxArgs& a, long long n, int side, int rowlo, int rowhi, int c0, int lane,
                                                   float acc[kNcnBwdChPerLane]) {
  const int lo = a.bt_ptr[side * a.N + n], hi = a.bt_ptr[side * a.N + n + 1];
  const int C = a.C;
  const bool decay = a.last_update != nullptr;
  for (int q0 = lo; q0 < hi; q0 += kWave) {  // (the bounds are the wave's: every lane takes every trip)
    const int q = q0 + lane;
    int r = 0, other = 0, m = 0;
    float w = 0.f;
    if (q < hi) {
      r = a.bt_r[q];
      // (both targets are inside [0, N): the keys kernel left every other pair out)
      other = (int)ld_idx(a.tar, a.tar_is64, side ? r : a.tar_stride + r);
      if (a.k == 4) {
        const long long ti = side ? other : n, tj = side ? n : other;
        const bool act = !a.last || (a.last[ti] == r && a.last[a.N + tj] == r);
        if (act) m = count_in(a.cols, rowlo, rowhi, other);  // A[i, j] = A[j, i]
        if (m) w = (float)m * (decay ? decay_weight(a.last_update, (long long)a.edge_time[r], n) : 1.f);
      }
    }
    const int cnt = hi - q0 < kWave ? hi - q0 : kWave;
    for (int b = 0; b < cnt; ++b) {
      const int rr = __shfl(r, b), oo = __shfl(other, b), mm = __shfl(m, b);
      const float ww = __shfl(w, b);
      const float* __restrict__ g0 = a.dxs + (long long)rr * a.lddxs + c0;
      const float* __restrict__ xo = a.x + (long long)oo * C + c0;
#pragma unroll
      for (int u = 0; u < kNcnBwdChPerLane; ++u) {
        const int c = lane + u * kWave;
        if (c0 + c < C) acc[u] = __fmaf_rn(g0[c], xo[c], acc[u]);
      }
      if (mm) {
        const float* __restrict__ gs = g0 + (long long)(1 + side) * C;
#pragma unroll
        for (int u = 0; u < kNcnBwdChPerLane; ++u) {
          const int c = lane + u * kWave;
          if (c0 + c < C) acc[u] = __fmaf_rn(ww, gs[c], acc[u]);
        }
      }
    }
  }
}

// term (3) of node n over the heads among the entries [slo, shi) of its row [rowlo, rowhi), channels [c0, c0 + 256): ascending a, then r
__device__ __forceinline__ void ncn_bwd_cn_terms(const DxArgs& a, long long n, int rowlo, int rowhi, int slo, int shi, int c0, int lane,
                                                 float acc[kNcnBwdChPerLane]) {
  const int32_t* __restrict__ cols = a.cols;
  const int C = a.C;
  const bool decay = a.last_update != nullptr;
  const float* __restrict__ gcn = a.dxs + (long long)(a.k - 1) * C + c0;
  for (int p0 = slo; p0 < shi; p0 += kWave) {
    const int p = p0 + lane;
    const bool in = p < shi;
    const int nb = in ? cols[p] : -1;
    const bool head = in && (p == rowlo || cols[p - 1] != nb);  // one visit per distinct id, by the chunk that holds the run's first entry
    int ma = 0, blo = 0, bhi = 0;
    if (head) {
      blo = a.bt_ptr[nb];
      bhi = a.bt_ptr[nb + 1];
      if (bhi > blo) ma = lower_bound_i32(cols, p, rowhi, (long long)nb + 1) - p;  // A[n, a]
    }
    unsigned long long heads = __ballot(ma > 0);
    while (heads) {  // ascending lanes = ascending ids
      const int hb = __ffsll((long long)heads) - 1;
      heads &= heads - 1;
      const int na = __shfl(nb, hb), lo = __shfl(blo, hb), hi = __shfl(bhi, hb);
      const float fa = (float)__shfl(ma, hb);
      for (int q0 = lo; q0 < hi; q0 += kWave) {
        const int q = q0 + lane;
        int r = 0;
        float w = 0.f;
        bool hit = false;
        if (q < hi) {
          r = a.bt_r[q];
          const long long tj = ld_idx(a.tar, a.tar_is64, a.tar_stride + r);  // (tar_i[r] = na; both inside [0, N))
          const bool act = !a.last || (a.last[na] == r && a.last[a.N + tj] == r);
          const int mb = act ? count_in(cols, rowlo, rowhi, tj) : 0;  // A[n, j]
          if (mb > 0) {
            hit = true;
            w = fa * (float)mb;
            if (decay) w *= decay_weight(a.last_update, (long long)a.edge_time[r], n);
          }
        }
        unsigned long long hits = __ballot(hit);
        while (hits) {  // ascending lanes = ascending r
          const int b = __ffsll((long long)hits) - 1;
          hits &= hits - 1;
          const int rr = __shfl(r, b);
          const float ww = __shfl(w, b);
          const float* __restrict__ g = gcn + (long long)rr * a.lddxs;
#pragma unroll
          for (int u = 0; u < kNcnBwdChPerLane; ++u) {
            const int c = lane + u * kWave;
            if (c0 + c < C) acc[u] = __fmaf_rn(ww, g[c], acc[u]);
          }
        }
      }
    }
  }
}

// a wave per node: terms (1) and (2), and term (3) of every row that is not long; every row of dx is written
__global__ __launch_bounds__(kNcnBwdThreads) void ncn_bwd_node_kernel(DxArgs a) {
  const int lane = lane_id();
  const long long nwaves = (long long)gridDim.x * kNcnBwdWaves;
  for (long long n = (long long)blockIdx.x * kNcnBwdWaves + threadIdx.x / kWave; n < a.N; n += nwaves) {
    const int rowlo = a.indptr[n], rowhi = a.indptr[n + 1];
    for (int c0 = 0; c0 < a.C; c0 += kWave * kNcnBwdChPerLane) {
      float acc[kNcnBwdChPerLane] = {0.f, 0.f, 0.f, 0.f};
      ncn_bwd_pair_terms(a, n, 0, rowlo, rowhi, c0, lane, acc);
      ncn_bwd_pair_terms(a, n, 1, rowlo, rowhi, c0, lane, acc);
      if (rowhi - rowlo <= a.long_row) ncn_bwd_cn_terms(a, n, rowlo, rowhi, rowlo, rowhi, c0, lane, acc);
#pragma unroll
      for (int u = 0; u < kNcnBwdChPerLane; ++u) {
        const int c = c0 + lane + u * kWave;
        if (c < a.C) a.dx[n * a.C + c] = acc[u];
      }
    }
  }
}

// the row that holds entry e < indptr[N]
__device__ __forceinline__ int ncn_bwd_row_of(const int32_t* __restrict__ indptr, int N, int e) {
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = (int)(((long long)lo + hi) >> 1);
    if (indptr[mid + 1] <= e) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// a wave per chunk of the entry array: term (3) over the chunk's part of the long rows that hold its first entry (slot 0) and its last (slot 1)
__global__ __launch_bounds__(kNcnBwdThreads) void ncn_bwd_chunk_kernel(DxArgs a, long long chunks) {
  const int lane = lane_id();
  const long long b = (long long)blockIdx.x * kNcnBwdWaves + threadIdx.x / kWave;
  const int N = (int)a.N, nnz = a.indptr[N];
  const long long e0l = b * kNcnBwdChunk;
  if (b >= chunks || e0l >= nnz) return;
  const int e0 = (int)e0l, e1 = (int)(e0l + kNcnBwdChunk < nnz ? e0l + kNcnBwdChunk : nnz);
  const int rA = ncn_bwd_row_of(a.indptr, N, e0), rB = ncn_bwd_row_of(a.indptr, N, e1 - 1);
  for (int slot = 0; slot < 2; ++slot) {
    const int r = slot ? rB : rA;
    if (slot && rB == rA) break;
    const int lo = a.indptr[r], hi = a.indptr[r + 1];
    if (hi - lo <= a.long_row) continue;
    const int slo = lo > e0 ? lo : e0, shi = hi < e1 ? hi : e1;
    float* __restrict__ dst = a.scratch + (b * 2 + slot) * a.C;
    for (int c0 = 0; c0 < a.C; c0 += kWave * kNcnBwdChPerLane) {
      float acc[kNcnBwdChPerLane] = {0.f, 0.f, 0.f, 0.f};
      ncn_bwd_cn_terms(a, r, lo, hi, slo, shi, c0, lane, acc);
#pragma unroll
      for (int u = 0; u < kNcnBwdChPerLane; ++u) {
        const int c = c0 + lane + u * kWave;
        if (c < a.C) dst[c] = acc[u];
      }
    }
  }
}

// a long row: its chunks' sums in ascending chunk order onto the terms (1) and (2) the node launch stored; a wave per node
__global__ __launch_bounds__(kNcnBwdThreads) void ncn_bwd_join_kernel(DxArgs a) {
  const int lane = lane_id();
  const long long n = (long long)blockIdx.x * kNcnBwdWaves + threadIdx.x / kWave;
  if (n >= a.N) return;
  const int lo = a.indptr[n], hi = a.indptr[n + 1];
  if (hi - lo <= a.long_row) return;
  for (int c = lane; c < a.C; c += kWave) {
    float acc = a.dx[n * a.C + c];
    for (int b = lo / kNcnBwdChunk; b <= (hi - 1) / kNcnBwdChunk; ++b) {
      const int slot = b * kNcnBwdChunk >= lo ? 0 : 1;  // the row holds the chunk's first entry, or it starts inside the chunk and holds its last
      acc = __fadd_rn(acc, a.scratch[((long long)b * 2 + slot) * a.C + c]);
    }
    a.dx[n * a.C + c] = acc;
  }
}

static size_t ncn_bwd_chunks(long long E) { return 2 * E > kNcnBwdLongRow ? (size_t)((2 * E + kNcnBwdChunk - 1) / kNcnBwdChunk) : 0; }

struct DxWorkspace {
  unsigned long long *k_in, *k_out;
  char* temp;
  size_t temp_bytes;
  int32_t *bt_ptr, *bt_r;
  float* scratch;
  size_t total;
};
static int dx_carve(void* workspace, long long N, long long E, long long B, int C, DxWorkspace& w) {
  WorkspaceCarver c(workspace);
  const size_t n = (size_t)(B > 0 ? 2 * B : 1);
  w.k_in = c.take<unsigned long long>(n);
  w.k_out = c.take<unsigned long long>(n);
  w.temp_bytes = 0;
  if (rocprim::radix_sort_keys(nullptr, w.temp_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, n, 0u, 64u) != hipSuccess)
    return TGMX_E_LAUNCH;
  w.temp = c.take<char>(w.temp_bytes);
  w.bt_ptr = c.take<int32_t>((size_t)(2 * N + 1));
  w.bt_r = c.take<int32_t>(n);
  w.scratch = c.take<float>(ncn_bwd_chunks(E) * 2 * (size_t)C);
  w.total = c.total();
  return TGMX_OK;
}
static bool dx_sizes_ok(long long N, long long E, long long B, int C, int k) {
  return (k == 2 || k == 4) && C > 0 && N > 0 && 2 * N < (1ll << 31) && E >= 0 && 2 * E < (1ll << 31) && B >= 0 && 2 * B < (1ll << 31);
}

static bool ncn_tail_route(int out_ch, int H) { return out_ch <= kNcnBwdMaxTail && (int64_t)out_ch * H * sizeof(float) <= 48 * 1024; }

}  // namespace tgmx

using namespace tgmx;

extern "C" size_t tgmx_ncn_dx_workspace_bytes(int64_t N, int64_t E, int64_t B, int32_t C) {
  DxWorkspace w;
  if (!dx_sizes_ok(N, E, B, C, 2)) return 0;
  return dx_carve(nullptr, N, E, B, C, w) == TGMX_OK ? w.total : 0;
}

extern "C" int tgmx_ncn_dx(const float* x, int64_t N, int32_t C, int32_t k, const int32_t* indptr, const int32_t* cols, int64_t E, const void* tar,
                           int32_t tar_is64, int64_t tar_stride, int64_t B, const int64_t* last_update, const int64_t* edge_time,
                           const int32_t* last, const float* dxs, int64_t lddxs, float* dx, void* workspace, size_t workspace_bytes,
                           tgmx_stream_t stream) {
  TGMX_REQUIRE(dx_sizes_ok(N, E, B, C, k) && tar_stride >= B && lddxs >= (int64_t)k * C,
               "ncn_dx: bad sizes k=%d (2 or 4) C=%d N=%lld E=%lld B=%lld lddxs=%lld", k, C, (long long)N, (long long)E, (long long)B, (long long)lddxs);
  TGMX_REQUIRE(dx && indptr && (E == 0 || cols), "ncn_dx: null pointer");
  TGMX_REQUIRE((last_update == nullptr) == (edge_time == nullptr), "ncn_dx: time decay needs last_update and edge_time");
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {  // no pair: every row is zero
    if (hipMemsetAsync(dx, 0, (size_t)N * C * sizeof(float), st) != hipSuccess) {
      set_error("ncn_dx: clearing dx failed");
      return TGMX_E_LAUNCH;
    }
    return TGMX_OK;
  }
  TGMX_REQUIRE(x && tar && dxs && workspace, "ncn_dx: null pointer");
  DxWorkspace w;
  if (dx_carve(workspace, N, E, B, C, w) != TGMX_OK || workspace_bytes < w.total) {
    set_error("ncn_dx: workspace too small (%zu bytes)", workspace_bytes);
    return TGMX_E_INVALID;
  }
  const int cb = col_bits(2 * N > B ? 2 * N : B);
  const long long n = 2 * B;
  hipLaunchKernelGGL(ncn_bwd_keys_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, st, tar, tar_is64 ? 1 : 0, (long long)tar_stride, (long long)B,
                     (long long)N, cb, w.k_in);
  TGMX_CHECK_LAUNCH("ncn_dx(keys)");
  if (rocprim::radix_sort_keys(w.temp, w.temp_bytes, (const unsigned long long*)w.k_in, w.k_out, (size_t)n, 0u, (unsigned)(2 * cb + 1), st) !=
      hipSuccess) {
    set_error("ncn_dx: radix sort failed");
    return TGMX_E_LAUNCH;
  }
  csr_rows_launch(w.k_out, n, 2 * (long long)N, cb, w.bt_ptr, w.bt_r, NoEntryValue{}, st);
  TGMX_CHECK_LAUNCH("ncn_dx(rows)");
  const size_t chunks = ncn_bwd_chunks(E);
  DxArgs a{x, (long long)N, C, k, indptr, cols, tar, tar_is64 ? 1 : 0, (long long)tar_stride, (long long)B, last_update, edge_time, last, dxs,
           (long long)lddxs, w.bt_ptr, w.bt_r, dx, chunks ? kNcnBwdLongRow : 0x7fffffff, chunks ? w.scratch : nullptr};
  hipLaunchKernelGGL(ncn_bwd_node_kernel, dim3(grid_for(N, kNcnBwdWaves, 16384)), dim3(kNcnBwdThreads), 0, st, a);
  TGMX_CHECK_LAUNCH("ncn_dx(nodes)");
  if (chunks) {
    hipLaunchKernelGGL(ncn_bwd_chunk_kernel, dim3((unsigned)((chunks + kNcnBwdWaves - 1) / kNcnBwdWaves)), dim3(kNcnBwdThreads), 0, st, a,
                       (long long)chunks);
    TGMX_CHECK_LAUNCH("ncn_dx(chunks)");
    hipLaunchKernelGGL(ncn_bwd_join_kernel, dim3((unsigned)((N + kNcnBwdWaves - 1) / kNcnBwdWaves)), dim3(kNcnBwdThreads), 0, st, a);
    TGMX_CHECK_LAUNCH("ncn_dx(join)");
  }
  return TGMX_OK;
}

// ---- the whole backward ---------------------------------------------------------------------------------------------------------------------
static int ncn_bwd_check(const tgmx_ncn_bwd_t* t, const char* who) {
  TGMX_REQUIRE(t, "%s: null argument block", who);
  const tgmx_ncn_fwd_t& a = t->fwd;
  TGMX_REQUIRE(dx_sizes_ok(a.N, a.E, a.B, a.C, a.k) && a.H > 0 && a.out_ch > 0 && a.ldxs >= (int64_t)a.k * a.C && a.ldh >= a.H && a.tar_stride >= a.B,
               "%s: bad sizes k=%d C=%d H=%d out=%d N=%lld E=%lld B=%lld", who, a.k, a.C, a.H, a.out_ch, (long long)a.N, (long long)a.E, (long long)a.B);
  return TGMX_OK;
}

// One walk over the backward; dry: only the workspace is laid out (*need = its bytes), nothing is launched
static int ncn_backward_pass(const tgmx_ncn_bwd_t* t, bool dry, size_t* need, tgmx_stream_t stream) {
  const tgmx_ncn_fwd_t& a = t->fwd;
  const int H = a.H, O = a.out_ch, K = a.k * a.C;
  const int64_t B = a.B;
  int rc;
#define RUN(call)                         \
  do {                                    \
    if (!dry && (rc = (call))) return rc; \
  } while (0)
  WorkspaceCarver ws(dry ? nullptr : t->workspace);
  const bool want_dpre = t->d_x || t->d_w1 || t->d_b1;
  const bool tail = ncn_tail_route(O, H);
  float* dpre = ws.take<float>(want_dpre ? (size_t)B * H : 0);
  float* dxs = ws.take<float>(t->d_x ? (size_t)B * K : 0);
  // the weights as the NT GEMMs of the dX steps read them: one launch
  float* w2t = ws.take<float>(want_dpre && !tail ? (size_t)H * O : 0);
  float* w1t = ws.take<float>(t->d_x ? (size_t)K * H : 0);
  {
    tgmx_pack_job_t jobs[2];
    int n = 0;
    if (want_dpre && !tail) jobs[n++] = tgmx_pack_job_t{a.w2, w2t, H, O, H, O, H, O, 1, 0};
    if (t->d_x) jobs[n++] = tgmx_pack_job_t{a.w1, w1t, K, H, K, H, K, H, 1, 0};
    if (n) RUN(tgmx_pack2d(jobs, n, stream));
  }
  const auto tn = [&](const float* A, int64_t lda, const float* Bm, int64_t ldb, float* C, int64_t ldc, int M, int N) -> int {
    float* part = ws.take<float>(tgmx_sgemm_tn_workspace_bytes(B, M, N, 1) / sizeof(float));
    return dry ? TGMX_OK : tgmx_sgemm_tn(A, lda, Bm, ldb, C, ldc, B, M, N, 1, 0, 0, 0, 0, part, stream);
  };
  const auto colsum = [&](const float* X, int64_t ld, int C, float* out) -> int {
    float* part = ws.take<float>((size_t)256 * C);
    return dry ? TGMX_OK : tgmx_colsum(X, ld, B, C, out, 0, part, stream);
  };
  // the last layer: dW2, db2, and dpre = (h > 0) * dout W2 (the mask is read from the saved h)
  if (tail) {
    const size_t floats = (t->d_w2 || t->d_b2) ? tgmx_decoder_tail_bwd_workspace_floats(B, H, O) : 0;
    float* part = ws.take<float>(floats);
    RUN(tgmx_decoder_tail_bwd(t->dout, t->lddout, a.h, a.ldh, B, H, a.w2, O, 1, want_dpre ? dpre : nullptr, H, t->d_w2, t->d_b2, part, floats, stream));
  } else {
    if (t->d_w2 && (rc = tn(t->dout, t->lddout, a.h, a.ldh, t->d_w2, H, O, H))) return rc;
    if (t->d_b2 && (rc = colsum(t->dout, t->lddout, O, t->d_b2))) return rc;
    if (want_dpre) {
      RUN(tgmx_sgemm_nt(t->dout, t->lddout, w2t, O, dpre, H, B, H, O, nullptr, 0, 1, 0, 0, 0, stream));
      RUN(tgmx_relu_mask(dpre, H, a.h, a.ldh, B, H, stream));
    }
  }
  // the first layer, in the parameters' own layouts
  if (t->d_w1 && (rc = tn(dpre, H, a.xs, a.ldxs, t->d_w1, K, H, K))) return rc;
  if (t->d_b1 && (rc = colsum(dpre, H, H, t->d_b1))) return rc;
  if (t->d_x) {
    RUN(tgmx_sgemm_nt(dpre, H, w1t, H, dxs, K, B, K, H, nullptr, 0, 1, 0, 0, 0, stream));
    const size_t bytes = tgmx_ncn_dx_workspace_bytes(a.N, a.E, B, a.C);
    if (bytes == 0) return TGMX_E_INVALID;
    char* dws = ws.take<char>(bytes);
    RUN(tgmx_ncn_dx(a.x, a.N, a.C, a.k, a.indptr, a.cols, a.E, a.tar, a.tar_is64, a.tar_stride, B, a.decay ? a.last_update : nullptr,
                    a.decay ? a.edge_time : nullptr, a.dup_all ? nullptr : a.last, dxs, K, t->d_x, dws, bytes, stream));
  }
#undef RUN
  *need = ws.total();
  return TGMX_OK;
}

extern "C" size_t tgmx_ncn_backward_workspace_bytes(const tgmx_ncn_bwd_t* t) {
  size_t need = 0;
  if (ncn_bwd_check(t, "ncn_backward_workspace_bytes") != TGMX_OK) return 0;
  return ncn_backward_pass(t, true, &need, nullptr) == TGMX_OK ? need : 0;
}

extern "C" int tgmx_ncn_backward(const tgmx_ncn_bwd_t* t, tgmx_stream_t stream) {
  int rc;
  if ((rc = ncn_bwd_check(t, "ncn_backward"))) return rc;
  const tgmx_ncn_fwd_t& a = t->fwd;
  const int K = a.k * a.C;
  if (a.B == 0) {  // no pair: every gradient asked for is zero
    hipStream_t st = (hipStream_t)stream;
    const struct { float* p; size_t n; } z[5] = {{t->d_x, (size_t)a.N * a.C}, {t->d_w1, (size_t)a.H * K}, {t->d_b1, (size_t)a.H},
                                                {t->d_w2, (size_t)a.out_ch * a.H}, {t->d_b2, (size_t)a.out_ch}};
    for (const auto& e : z)
      if (e.p && hipMemsetAsync(e.p, 0, e.n * sizeof(float), st) != hipSuccess) {
        set_error("ncn_backward: clearing a gradient failed");
        return TGMX_E_LAUNCH;
      }
    return TGMX_OK;
  }
  TGMX_REQUIRE(t->dout && t->lddout >= a.out_ch, "ncn_backward: no upstream gradient");
  TGMX_REQUIRE(a.x && a.tar && a.w1 && a.w2 && a.xs && a.h && a.indptr && (a.dup_all || a.last) && (!a.decay || (a.last_update && a.edge_time)),
               "ncn_backward: null pointer");
  size_t need = 0;
  if ((rc = ncn_backward_pass(t, true, &need, nullptr))) return rc;
  TGMX_REQUIRE(t->workspace && t->workspace_bytes >= need, "ncn_backward: workspace too small (%zu bytes, %zu needed)", t->workspace_bytes, need);
  return ncn_backward_pass(t, false, &need, stream);
}
