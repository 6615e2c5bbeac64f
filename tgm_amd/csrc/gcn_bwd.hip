// The backward of GCNConv and of the TGCN cell over a sparse adjacency (gcn.hip holds the normalisation and the propagate, tgcn.hip the cell's
// forward and its element-wise backward kernels) for gfx950: the transpose of a CSR, GCNConv's backward as one call, the cell's as one call.
//
// Transpose: the builder of edge_csr.h once more, with the entries of a finished CSR as its edge list.  Entry j of row i becomes the key
// (cols[j] << cb | i) carrying j; an entry slot behind the rows (the forward builder leaves dropped edges there) gets the key behind every
// row.  ONE stable radix sort, row pointers by binary search (csr_rows_kernel), cols_t = the key's low half, vals_t[u] = vals[pos[u]]: the
// values are COPIED, so the (row, col, value) triples are the forward's with row and col swapped, bit for bit, and equal (row, col) entries
// keep the forward's entry order.  How many entries are valid is read from indptr[N] on the device.  No float atomics anywhere: the
// propagate over the result (tgmx_gcn_propagate, no bias, no epilogue) gives the same bits on every run.
#include "common.h"
#include "edge_csr.h"
#include "spmm.h"

namespace tgmx {

// one wave per row: the row's entries get their row index (no search: the row is known, the lanes stride over its entries); then the slots
// behind the rows.  A row of the forward CSR is a destination's in-edges, so a hub costs its one wave len / 64 trips.
__global__ __launch_bounds__(kSpmmThreads) void csr_transpose_keys_kernel(const int32_t* __restrict__ indptr, const int32_t* __restrict__ cols,
                                                                          long long N, long long cap, int cb, unsigned long long* __restrict__ kd,
                                                                          unsigned* __restrict__ pos) {
  const int lane = lane_id();
  const long long nwaves = (long long)gridDim.x * kSpmmWaves;
  for (long long i = (long long)blockIdx.x * kSpmmWaves + threadIdx.x / kWave; i < N; i += nwaves) {
    const long long lo = indptr[i], hi = indptr[i + 1];
    for (long long j = lo + lane; j < hi && j < cap; j += kWave) {
      kd[j] = key_of(true, cols[j], i, cb);
      pos[j] = (unsigned)j;
    }
  }
  const long long nnz = indptr[N];
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long j = (nnz < 0 ? 0 : nnz) + (long long)blockIdx.x * blockDim.x + threadIdx.x; j < cap; j += step) {
    kd[j] = key_behind(cb);
    pos[j] = (unsigned)j;
  }
}

struct CopyValue {
  const float* vals;
  const unsigned* pos;
  float* vals_t;
  __device__ __forceinline__ void operator()(long long t, long long, long long) const { vals_t[t] = vals[pos[t]]; }
};

struct TransposeWorkspace {
  unsigned long long *kd_in, *kd_out;
  unsigned *pos_in, *pos_out;
  char* temp;
  size_t temp_bytes, total;
};
static int transpose_carve(void* workspace, long long cap, TransposeWorkspace& w) {
  WorkspaceCarver c(workspace);
  const size_t n = (size_t)(cap > 0 ? cap : 1);
  w.kd_in = c.take<unsigned long long>(n);
  w.kd_out = c.take<unsigned long long>(n);
  w.pos_in = c.take<unsigned>(n);
  w.pos_out = c.take<unsigned>(n);
  if (sort_keys_pos_temp_bytes(n, w.temp_bytes) != hipSuccess) return TGMX_E_LAUNCH;
  w.temp = c.take<char>(w.temp_bytes);
  w.total = c.total();
  return TGMX_OK;
}

// dG[i, g C + c] = dcat_g[i, c] (the left halves of the three gates' input gradients side by side: the operand of the one propagate)
__global__ __launch_bounds__(256) void tgcn_gather_left_kernel(const float* __restrict__ d0, const float* __restrict__ d1, const float* __restrict__ d2,
                                                               int C, long long N, float* __restrict__ dG) {
  const long long total = N * 3 * C;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += step) {
    const long long i = p / (3 * C);
    const int r = (int)(p - i * 3 * C), g = r / C, c = r - g * C;
    const float* d = g == 0 ? d0 : (g == 1 ? d1 : d2);
    dG[p] = d[i * 2 * C + c];
  }
}

}  // namespace tgmx

using namespace tgmx;

extern "C" size_t tgmx_csr_transpose_workspace_bytes(int64_t nnz, int64_t N) {
  TransposeWorkspace w;
  if (nnz < 0 || nnz >= (1ll << 31) || N <= 0 || N >= (1ll << 31)) return 0;
  return transpose_carve(nullptr, nnz, w) == TGMX_OK ? w.total : 0;
}

extern "C" int tgmx_csr_transpose(const int32_t* indptr, const int32_t* cols, const float* vals, const float* diag, int64_t N, int64_t nnz,
                                  int32_t* indptr_t, int32_t* cols_t, float* vals_t, float* diag_t, void* workspace, size_t workspace_bytes,
                                  tgmx_stream_t stream) {
  TGMX_REQUIRE(nnz >= 0 && nnz < (1ll << 31) && N > 0 && N < (1ll << 31), "csr_transpose: bad sizes nnz=%lld N=%lld", (long long)nnz, (long long)N);
  TGMX_REQUIRE(indptr && indptr_t && workspace && (nnz == 0 || (cols && vals && cols_t && vals_t)) && (!diag_t || diag), "csr_transpose: null pointer");
  hipStream_t st = (hipStream_t)stream;
  TransposeWorkspace l;
  if (transpose_carve(workspace, nnz, l) != TGMX_OK || workspace_bytes < l.total) {
    set_error("csr_transpose: workspace too small (%zu bytes)", workspace_bytes);
    return TGMX_E_INVALID;
  }
  const int cb = col_bits(N);
  if (nnz > 0) {  // (a zero-length sort is not issued)
    hipLaunchKernelGGL(csr_transpose_keys_kernel, dim3(grid_for(N, kSpmmWaves, 4096)), dim3(kSpmmThreads), 0, st, indptr,
                       cols, (long long)N, (long long)nnz, cb, l.kd_in, l.pos_in);
    TGMX_CHECK_LAUNCH("csr_transpose(keys)");
    if (sort_keys_pos(l.temp, l.temp_bytes, l.kd_in, l.kd_out, l.pos_in, l.pos_out, (size_t)nnz, cb, st) != hipSuccess) {
      set_error("csr_transpose: radix sort failed");
      return TGMX_E_LAUNCH;
    }
  }
  csr_rows_launch(l.kd_out, (long long)nnz, (long long)N, cb, indptr_t, cols_t, CopyValue{vals, l.pos_out, vals_t}, st);
  TGMX_CHECK_LAUNCH("csr_transpose(rows)");
  if (diag_t && diag_t != diag && hipMemcpyAsync(diag_t, diag, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
    set_error("csr_transpose: copying the diagonal failed");
    return TGMX_E_LAUNCH;
  }
  return TGMX_OK;
}

// ---- what the two backward calls share: A_hat^T as handed in, or built into the workspace ---------------------------------------------------
struct TransposedCsr {
  const int32_t *indptr, *cols;
  const float* vals;
};
// dry: carve only.  built: the caller's transposed CSR is used as it stands.
static int transposed_csr(WorkspaceCarver& ws, bool dry, const int32_t* indptr, const int32_t* cols, const float* vals, const float* diag, int64_t N,
                          int64_t nnz, const int32_t* indptr_t, const int32_t* cols_t, const float* vals_t, TransposedCsr& t, tgmx_stream_t stream) {
  if (indptr_t) {
    t = TransposedCsr{indptr_t, cols_t, vals_t};
    return TGMX_OK;
  }
  const size_t e1 = (size_t)(nnz > 0 ? nnz : 1);
  int32_t* ip = ws.take<int32_t>((size_t)N + 1);
  int32_t* ct = ws.take<int32_t>(e1);
  float* vt = ws.take<float>(e1);
  const size_t bytes = tgmx_csr_transpose_workspace_bytes(nnz, N);
  TGMX_REQUIRE(bytes > 0, "csr_transpose: %lld entries over %lld nodes are out of range", (long long)nnz, (long long)N);
  char* tw = ws.take<char>(bytes);
  t = TransposedCsr{ip, ct, vt};
  return dry ? TGMX_OK : tgmx_csr_transpose(indptr, cols, vals, diag, N, nnz, ip, ct, vt, nullptr, tw, bytes, stream);
}

#define RUN(call)                         \
  do {                                    \
    if (!dry && (rc = (call))) return rc; \
  } while (0)

// ---- GCNConv ------------------------------------------------------------------------------------------------------------------------------
static int gcn_conv_bwd_check(const tgmx_gcn_conv_bwd_t* a, const char* what) {
  TGMX_REQUIRE(a, "%s: null argument block", what);
  TGMX_REQUIRE(a->N > 0 && a->N < (1ll << 31) && a->C > 0 && a->C < (1 << 28) && a->in_ch > 0 && a->nnz >= 0 && a->nnz < (1ll << 31), "%s: bad sizes", what);
  TGMX_REQUIRE(a->lddo >= a->C, "%s: leading dimension of the upstream gradient below C", what);
  TGMX_REQUIRE(!a->d_x || (a->WT && a->ldwt >= a->C), "%s: d_x needs the transposed weight", what);
  TGMX_REQUIRE(!a->indptr_t || a->nnz == 0 || (a->cols_t && a->vals_t), "%s: the transposed CSR is incomplete", what);
  return TGMX_OK;
}

static int gcn_conv_backward_pass(const tgmx_gcn_conv_bwd_t* a, bool dry, size_t* need, tgmx_stream_t stream) {
  const int64_t N = a->N;
  const int C = a->C, in = a->in_ch;
  WorkspaceCarver ws(dry ? nullptr : a->workspace);
  int rc;
  if (a->d_b) {
    float* part = ws.take<float>((size_t)256 * C);
    RUN(tgmx_colsum(a->dout, a->lddo, N, C, a->d_b, 0, part, stream));
  }
  if (a->d_W || a->d_x) {
    TransposedCsr t;
    if ((rc = transposed_csr(ws, dry, a->indptr, a->cols, a->vals, a->diag, N, a->nnz, a->indptr_t, a->cols_t, a->vals_t, t, stream))) return rc;
    const long long ldy = (C + 3) / 4 * 4;
    float* dY = ws.take<float>((size_t)N * ldy);
    const size_t prop_floats = tgmx_cheb_propagate_scratch_floats(a->nnz, C);
    float* prop = ws.take<float>(prop_floats);
    RUN(tgmx_gcn_propagate(t.indptr, t.cols, t.vals, a->diag, N, C, a->dout, a->lddo, nullptr, TGMX_GCN_EPI_NONE, nullptr, 0, 0.f, nullptr, nullptr, 0, dY,
                           ldy, a->nnz, prop_floats ? prop : nullptr, prop_floats, stream));
    if (a->d_W) {
      float* part = ws.take<float>(tgmx_sgemm_tn_workspace_bytes(N, C, in, 1) / sizeof(float) + 1);
      RUN(tgmx_sgemm_tn(dY, ldy, a->x, a->ldx, a->d_W, in, N, C, in, 1, 0, 0, 0, 0, part, stream));
    }
    if (a->d_x) RUN(tgmx_sgemm_nt(dY, ldy, a->WT, a->ldwt, a->d_x, in, N, in, C, nullptr, 0, 1, 0, 0, 0, stream));
  }
  *need = ws.total();
  return TGMX_OK;
}

extern "C" size_t tgmx_gcn_conv_backward_csr_workspace_bytes(const tgmx_gcn_conv_bwd_t* a) {
  size_t need = 0;
  if (gcn_conv_bwd_check(a, "gcn_conv_backward_csr_workspace_bytes") != TGMX_OK) return 0;
  return gcn_conv_backward_pass(a, true, &need, nullptr) == TGMX_OK ? need : 0;
}

extern "C" int tgmx_gcn_conv_backward_csr(const tgmx_gcn_conv_bwd_t* a, tgmx_stream_t stream) {
  int rc;
  if ((rc = gcn_conv_bwd_check(a, "gcn_conv_backward_csr"))) return rc;
  TGMX_REQUIRE(a->dout && a->diag && (!(a->d_W) || (a->x && a->ldx >= a->in_ch)), "gcn_conv_backward_csr: null pointer or narrow x");
  TGMX_REQUIRE(a->indptr_t || (a->indptr && (a->nnz == 0 || (a->cols && a->vals))), "gcn_conv_backward_csr: the CSR is missing");
  size_t need = 0;
  if ((rc = gcn_conv_backward_pass(a, true, &need, nullptr))) return rc;
  TGMX_REQUIRE(a->workspace && a->workspace_bytes >= need, "gcn_conv_backward_csr: workspace too small (%zu bytes, %zu needed)", a->workspace_bytes, need);
  return gcn_conv_backward_pass(a, false, &need, stream);
}

// ---- the TGCN cell ------------------------------------------------------------------------------------------------------------------------
extern "C" int tgmx_tgcn_gather_left(const float* dcat_u, const float* dcat_r, const float* dcat_c, int32_t C, int64_t N, float* dG,
                                     tgmx_stream_t stream) {
  TGMX_REQUIRE(C > 0 && C < (1 << 27) && N >= 0 && N < (1ll << 31), "tgcn_gather_left: bad sizes");
  if (N == 0) return TGMX_OK;
  TGMX_REQUIRE(dcat_u && dcat_r && dcat_c && dG, "tgcn_gather_left: null pointer");
  hipLaunchKernelGGL(tgcn_gather_left_kernel, dim3(grid_for(N * 3 * C, 256, 16384)), dim3(256), 0, (hipStream_t)stream, dcat_u, dcat_r, dcat_c, C,
                     (long long)N, dG);
  TGMX_CHECK_LAUNCH("tgcn_gather_left");
  return TGMX_OK;
}

static int tgcn_csr_bwd_check(const tgmx_tgcn_csr_bwd_t* a, const char* what) {
  TGMX_REQUIRE(a, "%s: null argument block", what);
  TGMX_REQUIRE(a->N > 0 && a->N < (1ll << 31) && a->C > 0 && a->C < (1 << 27) && a->in_ch > 0 && a->nnz >= 0 && a->nnz < (1ll << 31), "%s: bad sizes", what);
  TGMX_REQUIRE(a->ldx >= a->in_ch, "%s: leading dimension of x below in_ch", what);
  TGMX_REQUIRE(!a->d_x || (a->W3T && a->ldw3t >= 3ll * a->C), "%s: d_x needs the transposed stacked weight", what);
  TGMX_REQUIRE(!a->indptr_t || a->nnz == 0 || (a->cols_t && a->vals_t), "%s: the transposed CSR is incomplete", what);
  return TGMX_OK;
}

static int tgcn_csr_backward_pass(const tgmx_tgcn_csr_bwd_t* a, bool dry, size_t* need, tgmx_stream_t stream) {
  const int64_t N = a->N;
  const int C = a->C, in = a->in_ch;
  WorkspaceCarver ws(dry ? nullptr : a->workspace);
  int rc;
  float* dpre[3];  // u, r, c
  for (int g = 0; g < 3; ++g) dpre[g] = ws.take<float>((size_t)N * C);
  float* dcat[3];
  for (int g = 0; g < 3; ++g) dcat[g] = ws.take<float>((size_t)N * 2 * C);
  float* dH = a->d_H ? a->d_H : ws.take<float>((size_t)N * C);
  const size_t tn_lin = tgmx_sgemm_tn_workspace_bytes(N, C, 2 * C, 1), tn_conv = tgmx_sgemm_tn_workspace_bytes(N, 3 * C, in, 1);
  float* tn_part = ws.take<float>((tn_lin > tn_conv ? tn_lin : tn_conv) / sizeof(float) + 1);  // (the two shapes of tgmx_sgemm_tn below, in turn)
  float* cs_part = ws.take<float>((size_t)256 * 3 * C);
  // 1. the output gate
  RUN(tgmx_tgcn_gate_backward(a->dout, a->pre[0], a->pre[2], a->H, N * C, dpre[0], dpre[2], dH, stream));
  // 2. d cat_g = d pre_g W_g, 3. the reset gate in between (lin_wT[g]: [2C, C])
  RUN(tgmx_sgemm_nt(dpre[0], C, a->lin_wT[0], C, dcat[0], 2 * C, N, 2 * C, C, nullptr, 0, 1, 0, 0, 0, stream));
  RUN(tgmx_sgemm_nt(dpre[2], C, a->lin_wT[2], C, dcat[2], 2 * C, N, 2 * C, C, nullptr, 0, 1, 0, 0, 0, stream));
  RUN(tgmx_tgcn_reset_backward(dcat[2], dcat[0], nullptr, a->pre[1], a->H, C, N, dpre[1], dH, stream));
  RUN(tgmx_sgemm_nt(dpre[1], C, a->lin_wT[1], C, dcat[1], 2 * C, N, 2 * C, C, nullptr, 0, 1, 0, 0, 0, stream));
  RUN(tgmx_tgcn_reset_backward(nullptr, nullptr, dcat[1], nullptr, nullptr, C, N, nullptr, dH, stream));
  // 4. the gates' Linear layers, each gradient in its parameter's layout
  for (int g = 0; g < 3; ++g) {
    if (a->d_lw[g]) RUN(tgmx_sgemm_tn(dpre[g], C, a->cat[g], 2 * C, a->d_lw[g], 2 * C, N, C, 2 * C, 1, 0, 0, 0, 0, tn_part, stream));
    if (a->d_lb[g]) RUN(tgmx_colsum(dpre[g], C, N, C, a->d_lb[g], 0, cs_part, stream));
  }
  if (!(a->d_W3 || a->d_b3 || a->d_x)) {
    *need = ws.total();
    return TGMX_OK;
  }
  // 5. dG = the left halves side by side, 6. db3
  const long long ldg = (3ll * C + 3) / 4 * 4;
  float* dG = ws.take<float>((size_t)N * 3 * C);
  RUN(tgmx_tgcn_gather_left(dcat[0], dcat[1], dcat[2], C, N, dG, stream));
  if (a->d_b3) RUN(tgmx_colsum(dG, 3 * C, N, 3 * C, a->d_b3, 0, cs_part, stream));
  if (a->d_W3 || a->d_x) {
    // 7. dY = A_hat^T dG
    TransposedCsr t;
    if ((rc = transposed_csr(ws, dry, a->indptr, a->cols, a->vals, a->diag, N, a->nnz, a->indptr_t, a->cols_t, a->vals_t, t, stream))) return rc;
    float* dY = ws.take<float>((size_t)N * ldg);
    const size_t prop_floats = tgmx_cheb_propagate_scratch_floats(a->nnz, 3 * C);
    float* prop = ws.take<float>(prop_floats);
    RUN(tgmx_gcn_propagate(t.indptr, t.cols, t.vals, a->diag, N, 3 * C, dG, 3 * C, nullptr, TGMX_GCN_EPI_NONE, nullptr, 0, 0.f, nullptr, nullptr, 0, dY, ldg,
                           a->nnz, prop_floats ? prop : nullptr, prop_floats, stream));
    // 8. dW3 = dY^T X, 9. dX = dY W3 (W3T: [in, 3C])
    if (a->d_W3) RUN(tgmx_sgemm_tn(dY, ldg, a->x, a->ldx, a->d_W3, in, N, 3 * C, in, 1, 0, 0, 0, 0, tn_part, stream));
    if (a->d_x) RUN(tgmx_sgemm_nt(dY, ldg, a->W3T, a->ldw3t, a->d_x, in, N, in, 3 * C, nullptr, 0, 1, 0, 0, 0, stream));
  }
  *need = ws.total();
  return TGMX_OK;
}
#undef RUN

extern "C" size_t tgmx_tgcn_backward_csr_workspace_bytes(const tgmx_tgcn_csr_bwd_t* a) {
  size_t need = 0;
  if (tgcn_csr_bwd_check(a, "tgcn_backward_csr_workspace_bytes") != TGMX_OK) return 0;
  return tgcn_csr_backward_pass(a, true, &need, nullptr) == TGMX_OK ? need : 0;
}

extern "C" int tgmx_tgcn_backward_csr(const tgmx_tgcn_csr_bwd_t* a, tgmx_stream_t stream) {
  int rc;
  if ((rc = tgcn_csr_bwd_check(a, "tgcn_backward_csr"))) return rc;
  TGMX_REQUIRE(a->dout && a->H && a->diag, "tgcn_backward_csr: null pointer");
  for (int g = 0; g < 3; ++g) TGMX_REQUIRE(a->cat[g] && a->pre[g] && a->lin_wT[g], "tgcn_backward_csr: the forward's saved buffers are missing (gate %d)", g);
  TGMX_REQUIRE(!(a->d_W3) || a->x, "tgcn_backward_csr: d_W3 needs x");
  TGMX_REQUIRE(a->indptr_t || (a->indptr && (a->nnz == 0 || (a->cols && a->vals))), "tgcn_backward_csr: the CSR is missing");
  size_t need = 0;
  if ((rc = tgcn_csr_backward_pass(a, true, &need, nullptr))) return rc;
  TGMX_REQUIRE(a->workspace && a->workspace_bytes >= need, "tgcn_backward_csr: workspace too small (%zu bytes, %zu needed)", a->workspace_bytes, need);
  return tgcn_csr_backward_pass(a, false, &need, stream);
}
