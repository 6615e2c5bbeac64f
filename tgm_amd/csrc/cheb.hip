// ChebConv and the GCLSTM cell (the reference's tgm/nn/encoder/gclstm.py) for gfx950: the scaled Laplacian of a snapshot as a CSR by
// destination, a gather SpMM over it, the LSTM gate epilogue, and the cell's inference forward as one call.  ChebConv is third-party to the
// reference (torch_geometric); it is implemented from its published definition (get_laplacian, then 2 L / lambda_max - I): parity unpinned
// upstream.
//
// Laplacian: the builder of edge_csr.h with keys (dst << cb | src).  Dropped: a self loop, and an edge with an endpoint outside [0, N).  The
// degree is taken over the SOURCE index: without weights it is an integer count (integer atomics do not depend on the order of arrival); with
// weights a second stable sort by source groups the positions and one wave per node sums its group in a fixed order.
//
// The transpose (tgmx_cheb_laplacian_t, the backward's operator) is the same builder with the key roles swapped, (src << cb | dst): the
// degrees, ChebEntry's arithmetic and the diagonal are the very same code, so its entries are those of the forward's CSR bit for bit.
//
// Propagate: out = alpha (L_hat t) + beta prev, the gather kernels of spmm.h (shared with gcn.hip) with ChebEpi as their epilogue.
#include "common.h"
#include "edge_csr.h"
#include "spmm.h"

namespace tgmx {

constexpr int kChebThreads = kSpmmThreads;
constexpr int kChebWaves = kSpmmWaves;

// ---- Laplacian --------------------------------------------------------------------------------------------------------------------------
// keys by destination, or by source for the transpose (and by source when the degrees are weighted); cnt: the unweighted degree as an
// integer count
__global__ __launch_bounds__(256) void cheb_keys_kernel(const void* __restrict__ src, const void* __restrict__ dst, int is64, long long E, long long N,
                                                        int cb, int by_src, unsigned long long* __restrict__ kd, unsigned* __restrict__ pos,
                                                        unsigned* __restrict__ ks, int* __restrict__ cnt, int* __restrict__ skipped) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += step) {
    const long long s = ld_idx(src, is64, e), d = ld_idx(dst, is64, e);
    const bool in = s >= 0 && s < N && d >= 0 && d < N;
    const bool ok = in && s != d;
    if (!in && skipped) atomicAdd(skipped, 1);
    kd[e] = by_src ? key_of(ok, s, d, cb) : key_of(ok, d, s, cb);
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
      const long long lo = key_lower_bound(ks_sorted, E, (unsigned)i);  // the node's group of the source-sorted keys: [lo, end)
      const long long end = lo + key_lower_bound(ks_sorted + lo, E - lo, (unsigned)i + 1);
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

// entry t of the Laplacian, from source s to destination d: -w_e scaled by the normalisation's degree factors, then 2 / lambda_max
// (by_src: the rows are the sources, so the key's column is the destination)
struct ChebEntry {
  const unsigned* pos_sorted;
  const float* w;
  const float* dis;
  int norm;
  float lambda_max;
  const float* lambda_ptr;
  float* vals;
  int by_src;
  __device__ __forceinline__ void operator()(long long t, long long col, long long row) const {
    const long long s = by_src ? row : col, d = by_src ? col : row;
    const float lmax = lambda_ptr ? lambda_ptr[0] : lambda_max;
    const float we = w ? w[pos_sorted[t]] : 1.f;
    float m;
    if (norm == TGMX_CHEB_NORM_SYM) m = dis[s] * we * dis[d];
    else if (norm == TGMX_CHEB_NORM_RW) m = dis[s] * we;
    else m = we;
    float v = (2.0f * -m) / lmax;
    if (isinf(v)) v = 0.f;
    vals[t] = v;
  }
};

struct ChebWorkspace {
  unsigned long long *kd_in, *kd_out;
  unsigned *pos_in, *pos_out, *ks_in, *ks_out, *ps_out;
  int* cnt;
  float* dis;
  char* temp;
  size_t temp_bytes, total;
};
static int cheb_carve(void* workspace, long long E, long long N, ChebWorkspace& w) {
  WorkspaceCarver c(workspace);
  const size_t n = (size_t)(E > 0 ? E : 1);
  w.kd_in = c.take<unsigned long long>(n);
  w.kd_out = c.take<unsigned long long>(n);
  w.pos_in = c.take<unsigned>(n);
  w.pos_out = c.take<unsigned>(n);
  w.ks_in = c.take<unsigned>(n);
  w.ks_out = c.take<unsigned>(n);
  w.ps_out = c.take<unsigned>(n);
  w.cnt = c.take<int>((size_t)N);
  w.dis = c.take<float>((size_t)N);
  size_t tb32 = 0;  // the sort by source: 32-bit keys
  if (sort_keys_pos_temp_bytes(n, w.temp_bytes) != hipSuccess) return TGMX_E_LAUNCH;
  if (rocprim::radix_sort_pairs(nullptr, tb32, (const unsigned*)nullptr, (unsigned*)nullptr, (const unsigned*)nullptr, (unsigned*)nullptr, n, 0u,
                                32u) != hipSuccess)
    return TGMX_E_LAUNCH;
  if (tb32 > w.temp_bytes) w.temp_bytes = tb32;
  w.temp = c.take<char>(w.temp_bytes);
  w.total = c.total();
  return TGMX_OK;
}

// ---- propagate ----------------------------------------------------------------------------------------------------------------------------
// the epilogue of the Chebyshev recurrence over the shared gather SpMM (spmm.h): out = alpha (L_hat t) + beta prev
struct ChebEpi {
  const float* prev;
  long long ldp;
  float alpha, beta;
  template <bool VEC>
  __device__ __forceinline__ void apply(long long i, int c0, int C, int lane, float o[kSpmmChPerLane]) const {
#pragma unroll
    for (int q = 0; q < kSpmmChPerLane; ++q) o[q] = alpha * o[q];
    if (beta != 0.f) {
      float p[kSpmmChPerLane];
      spmm_load<VEC>(prev + i * ldp, c0, C, lane, p);
#pragma unroll
      for (int q = 0; q < kSpmmChPerLane; ++q) o[q] = __fmaf_rn(beta, p[q], o[q]);
    }
  }
};

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
  ChebWorkspace w;
  if (E < 0 || E >= (1ll << 31) || N <= 0 || N >= (1ll << 31)) return 0;
  return cheb_carve(nullptr, E, N, w) == TGMX_OK ? w.total : 0;
}

// rows by destination (by_src = 0) or by source (the transpose); `what` names the entry point in the messages
static int cheb_laplacian_build(int by_src, const char* what, const void* src, const void* dst, int32_t idx64, const float* w, int64_t E, int64_t N,
                                int32_t normalization, float lambda_max, const float* lambda_ptr, int32_t* indptr, int32_t* cols, float* vals,
                                float* diag, void* workspace, size_t workspace_bytes, int32_t* skipped, tgmx_stream_t stream) {
  TGMX_REQUIRE(E >= 0 && E < (1ll << 31) && N > 0 && N < (1ll << 31), "%s: bad sizes E=%lld N=%lld", what, (long long)E, (long long)N);
  TGMX_REQUIRE(normalization >= TGMX_CHEB_NORM_NONE && normalization <= TGMX_CHEB_NORM_RW, "%s: unknown normalization %d", what, normalization);
  TGMX_REQUIRE(indptr && diag && workspace && (E == 0 || (src && dst && cols && vals)), "%s: null pointer", what);
  hipStream_t st = (hipStream_t)stream;
  ChebWorkspace l;
  if (cheb_carve(workspace, E, N, l) != TGMX_OK || workspace_bytes < l.total) {
    set_error("%s: workspace too small (%zu bytes)", what, workspace_bytes);
    return TGMX_E_INVALID;
  }
  const int cb = col_bits(N);
  const bool weighted = w != nullptr && E > 0;
  if (!weighted && hipMemsetAsync(l.cnt, 0, (size_t)N * sizeof(int), st) != hipSuccess) {
    set_error("%s: clearing the degree counts failed", what);
    return TGMX_E_LAUNCH;
  }
  if (E > 0) {  // (a zero-length sort is not issued)
    hipLaunchKernelGGL(cheb_keys_kernel, dim3(grid_for(E, 256, 4096)), dim3(256), 0, st, src, dst, idx64, (long long)E, (long long)N, cb, by_src, l.kd_in,
                       l.pos_in, weighted ? l.ks_in : nullptr, l.cnt, skipped);
    TGMX_CHECK_LAUNCH(what);
    if (weighted) {
      int sb = 1;
      while ((1ll << sb) <= N) ++sb;  // the keys go up to N itself (the skipped edges)
      size_t tb = l.temp_bytes;
      if (rocprim::radix_sort_pairs(l.temp, tb, (const unsigned*)l.ks_in, l.ks_out, (const unsigned*)l.pos_in, l.ps_out, (size_t)E, 0u, (unsigned)sb,
                                    st) != hipSuccess) {
        set_error("%s: radix sort (by source) failed", what);
        return TGMX_E_LAUNCH;
      }
    }
    if (sort_keys_pos(l.temp, l.temp_bytes, l.kd_in, l.kd_out, l.pos_in, l.pos_out, (size_t)E, cb, st) != hipSuccess) {
      set_error("%s: radix sort (of the rows) failed", what);
      return TGMX_E_LAUNCH;
    }
  }
  hipLaunchKernelGGL(cheb_degree_kernel, dim3(grid_for(N, kChebWaves, 4096)), dim3(kChebThreads), 0, st, weighted ? l.ks_out : nullptr, l.ps_out, w,
                     l.cnt, (long long)E, (long long)N, normalization, lambda_max, lambda_ptr, l.dis, diag);
  TGMX_CHECK_LAUNCH(what);
  csr_rows_launch(l.kd_out, (long long)E, (long long)N, cb, indptr, cols, ChebEntry{l.pos_out, w, l.dis, normalization, lambda_max, lambda_ptr, vals, by_src}, st);
  TGMX_CHECK_LAUNCH(what);
  return TGMX_OK;
}

extern "C" int tgmx_cheb_laplacian(const void* src, const void* dst, int32_t idx64, const float* w, int64_t E, int64_t N, int32_t normalization,
                                   float lambda_max, const float* lambda_ptr, int32_t* indptr, int32_t* cols, float* vals, float* diag,
                                   void* workspace, size_t workspace_bytes, int32_t* skipped, tgmx_stream_t stream) {
  return cheb_laplacian_build(0, "cheb_laplacian", src, dst, idx64, w, E, N, normalization, lambda_max, lambda_ptr, indptr, cols, vals, diag, workspace,
                              workspace_bytes, skipped, stream);
}

extern "C" int tgmx_cheb_laplacian_t(const void* src, const void* dst, int32_t idx64, const float* w, int64_t E, int64_t N, int32_t normalization,
                                     float lambda_max, const float* lambda_ptr, int32_t* indptr, int32_t* cols, float* vals, float* diag,
                                     void* workspace, size_t workspace_bytes, int32_t* skipped, tgmx_stream_t stream) {
  return cheb_laplacian_build(1, "cheb_laplacian_t", src, dst, idx64, w, E, N, normalization, lambda_max, lambda_ptr, indptr, cols, vals, diag,
                              workspace, workspace_bytes, skipped, stream);
}

extern "C" size_t tgmx_cheb_propagate_scratch_floats(int64_t nnz, int32_t C) { return spmm_scratch_floats(nnz, C); }

extern "C" int tgmx_cheb_propagate(const int32_t* indptr, const int32_t* cols, const float* vals, const float* diag, int64_t N, int32_t C,
                                   const float* t, int64_t ldt, const float* prev, int64_t ldp, float alpha, float beta, float* out, int64_t ldo,
                                   int64_t nnz, float* scratch, size_t scratch_floats, tgmx_stream_t stream) {
  TGMX_REQUIRE(N >= 0 && N < (1ll << 31) && C > 0 && ldt >= C && ldo >= C && (beta == 0.f || ldp >= C) && nnz >= 0 && nnz < (1ll << 31),
               "cheb_propagate: bad sizes N=%lld C=%d nnz=%lld", (long long)N, C, (long long)nnz);
  if (N == 0) return TGMX_OK;
  TGMX_REQUIRE(indptr && diag && t && out && (beta == 0.f || prev), "cheb_propagate: null pointer");
  SpmmArgs<ChebEpi> a{indptr, cols, vals, diag, (long long)N, C, t, (long long)ldt, out, (long long)ldo, 0, nullptr,
                      ChebEpi{prev, (long long)ldp, alpha, beta}};
  const bool vec = spmm_vec_ok(t, ldt) && spmm_vec_ok(out, ldo) && (beta == 0.f || spmm_vec_ok(prev, ldp));
  return spmm_run(a, nnz, scratch, scratch_floats, vec, "cheb_propagate", (hipStream_t)stream);
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
  hipLaunchKernelGGL(gclstm_operand_kernel, dim3(grid_for(N * fill, 256, 16384)), dim3(256), 0, st, a->x, in, a->H, C, (int)width, (long long)N,
                     a->op, (long long)a->ldop);
  TGMX_CHECK_LAUNCH("gclstm_forward(operand)");
  for (int k = 1; k < K; ++k) {  // Tx_1 = L_hat Tx_0;  Tx_k = 2 L_hat Tx_{k-1} - Tx_{k-2}
    float* tx = a->op + in + (long long)k * C;
    if ((rc = tgmx_cheb_propagate(a->indptr, a->cols, a->vals, a->diag, N, C, tx - C, a->ldop, k > 1 ? tx - 2 * C : nullptr, a->ldop,
                                  k > 1 ? 2.f : 1.f, k > 1 ? -1.f : 0.f, tx, a->ldop, a->E, a->prop_ws, a->prop_ws_floats, stream)))
      return rc;
  }
  if ((rc = tgmx_sgemm_nt(a->op, a->ldop, a->W, a->ldw, a->pre, 4 * C, N, 4 * C, (int32_t)width, a->b, 0, 1, 0, 0, 0, stream))) return rc;
  hipLaunchKernelGGL(gclstm_gates_kernel, dim3(grid_for(N * C, 256, 16384)), dim3(256), 0, st, a->pre, a->Cprev, C, (long long)N, a->H_out, a->C_out);
  TGMX_CHECK_LAUNCH("gclstm_forward(gates)");
  return TGMX_OK;
}
