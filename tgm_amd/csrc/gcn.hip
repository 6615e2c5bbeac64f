// GCNConv on a sparse adjacency and ROLAND (the reference's tgm/nn/encoder/roland.py) for gfx950: GCN's normalised adjacency
// D^-1/2 (A + I) D^-1/2 of a snapshot as a CSR by destination, the gather SpMM over it with the layer's bias, activation and embedding update
// as its epilogue, the GRU update's gates, and ROLAND's forward as one call.  GCNConv is third-party to the reference (torch_geometric); it
// is implemented from its published definition (gcn_norm with add_remaining_self_loops), as tgcn.hip's dense builder is: parity unpinned
// upstream.
//
// Normalisation: the builder of edge_csr.h with keys (dst << cb | src).  Dropped: an edge with an endpoint outside [0, N), and with
// add_self_loops an explicit self loop, which leaves its edge position in its node's slot by an integer max (the highest position wins,
// whatever the order of arrival).  One wave per node then finds the node's row (so indptr is written here, not by the shared rows kernel, and
// an empty edge list needs no further launch), takes the degree over the DESTINATION index -- the row's length without weights, with weights
// the row's weights summed in CSR order, lanes striding, folded in a fixed butterfly -- adds the loop weight and writes deg^-1/2 (in double:
// vals and diag are then exact values rounded once) and the diagonal.
//
// Propagate: the gather kernels of spmm.h (shared with cheb.hip) with GcnEpi as their epilogue.
#include "common.h"
#include "edge_csr.h"
#include "spmm.h"

namespace tgmx {

// ---- normalisation ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gcn_keys_kernel(const void* __restrict__ src, const void* __restrict__ dst, int is64, long long E, long long N,
                                                       int cb, int add_self_loops, unsigned long long* __restrict__ kd, unsigned* __restrict__ pos,
                                                       int* __restrict__ loop_e, int* __restrict__ skipped) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += step) {
    const long long s = ld_idx(src, is64, e), d = ld_idx(dst, is64, e);
    const bool in = s >= 0 && s < N && d >= 0 && d < N;
    const bool loop = in && add_self_loops && s == d;  // folded into the diagonal
    if (!in && skipped) atomicAdd(skipped, 1);
    if (loop) atomicMax(&loop_e[d], (int)e);
    kd[e] = key_of(in && !loop, d, s, cb);
    pos[e] = (unsigned)e;
  }
}

// one wave per node: indptr[i] (and indptr[N] by the last node), dinv[i] = deg^-1/2 (0 for deg = 0), diag[i] = dinv lw dinv.  The degree and
// its inverse root are kept in double, so that every float this builder hands out (vals, diag) is the exact value rounded ONCE.
__global__ __launch_bounds__(kSpmmThreads) void gcn_node_kernel(const unsigned long long* __restrict__ sorted, const unsigned* __restrict__ pos_sorted,
                                                                const float* __restrict__ w, const int* __restrict__ loop_e, long long E, long long N,
                                                                int cb, float fill, int add_self_loops, int32_t* __restrict__ indptr,
                                                                double* __restrict__ dinv, float* __restrict__ diag) {
  const int lane = lane_id();
  const long long nwaves = (long long)gridDim.x * kSpmmWaves;
  for (long long i = (long long)blockIdx.x * kSpmmWaves + threadIdx.x / kWave; i < N; i += nwaves) {
    const long long lo = key_lower_bound(sorted, E, key_row_start(i, cb));
    const long long hi = key_lower_bound(sorted, E, key_row_start(i + 1, cb));
    double deg;
    if (w) {
      double part = 0.0;
      for (long long j = lo + lane; j < hi; j += kWave) part += (double)w[pos_sorted[j]];
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) part += __shfl_xor(part, off);
      deg = part;
    } else {
      deg = (double)(hi - lo);
    }
    if (lane == 0) {
      double lw = 0.0;
      if (add_self_loops) {
        const int le = loop_e[i];
        lw = le < 0 ? (double)fill : (w ? (double)w[le] : 1.0);
      }
      const double d = deg + lw;
      const double f = d > 0.0 ? 1.0 / sqrt(d) : 0.0;
      dinv[i] = f;
      diag[i] = (float)(f * lw * f);
      indptr[i] = (int32_t)lo;
      if (i == N - 1) indptr[N] = (int32_t)hi;
    }
  }
}

__global__ __launch_bounds__(256) void gcn_entries_kernel(const unsigned long long* __restrict__ sorted, const unsigned* __restrict__ pos_sorted,
                                                          const float* __restrict__ w, const double* __restrict__ dinv, long long E, int cb,
                                                          int32_t* __restrict__ cols, float* __restrict__ vals) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < E; t += step) {
    const unsigned long long key = sorted[t];
    if (key >= key_behind(cb)) continue;
    const long long s = key_col(key, cb), d = key_row(key, cb);
    cols[t] = (int32_t)s;
    vals[t] = (float)(dinv[s] * (w ? (double)w[pos_sorted[t]] : 1.0) * dinv[d]);
  }
}

struct GcnWorkspace {
  unsigned long long *kd_in, *kd_out;
  unsigned *pos_in, *pos_out;
  int* loop_e;
  double* dinv;
  char* temp;
  size_t temp_bytes, total;
};
static int gcn_carve(void* workspace, long long E, long long N, GcnWorkspace& w) {
  WorkspaceCarver c(workspace);
  const size_t n = (size_t)(E > 0 ? E : 1);
  w.kd_in = c.take<unsigned long long>(n);
  w.kd_out = c.take<unsigned long long>(n);
  w.pos_in = c.take<unsigned>(n);
  w.pos_out = c.take<unsigned>(n);
  w.loop_e = c.take<int>((size_t)N);
  w.dinv = c.take<double>((size_t)N);
  if (sort_keys_pos_temp_bytes(n, w.temp_bytes) != hipSuccess) return TGMX_E_LAUNCH;
  w.temp = c.take<char>(w.temp_bytes);
  w.total = c.total();
  return TGMX_OK;
}

// ---- propagate ----------------------------------------------------------------------------------------------------------------------------
// o = s + bias;  RELU: relu(o);  TAU: tau prev[i] + (1 - tau) relu(o), prev[i] also stored to copy[i] when that is given
struct GcnEpi {
  const float* bias;
  int mode;
  const float* prev;
  long long ldp;
  float tau;
  const float* tau_ptr;
  float* copy;
  long long ldc;
  template <bool VEC>
  __device__ __forceinline__ void apply(long long i, int c0, int C, int lane, float o[kSpmmChPerLane]) const {
    if (bias) {
      float b[kSpmmChPerLane];
      spmm_load<VEC>(bias, c0, C, lane, b);
#pragma unroll
      for (int q = 0; q < kSpmmChPerLane; ++q) o[q] = __fadd_rn(o[q], b[q]);
    }
    if (mode == TGMX_GCN_EPI_NONE) return;
#pragma unroll
    for (int q = 0; q < kSpmmChPerLane; ++q) o[q] = o[q] < 0.f ? 0.f : o[q];
    if (mode != TGMX_GCN_EPI_TAU) return;
    const float tv = tau_ptr ? tau_ptr[0] : tau;
    float p[kSpmmChPerLane];
    spmm_load<VEC>(prev + i * ldp, c0, C, lane, p);
    if (copy) spmm_store<VEC>(copy + i * ldc, c0, C, lane, p);
#pragma unroll
    for (int q = 0; q < kSpmmChPerLane; ++q) o[q] = __fmaf_rn(tv, p[q], __fmul_rn(1.f - tv, o[q]));
  }
};

// ---- ROLAND's GRU update --------------------------------------------------------------------------------------------------------------------
// gi = h W_ih^T + b_ih, gh = prev W_hh^T + b_hh, [N, 3C] each in r, z, n order (torch.nn.GRUCell):
//   r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r gh_n), h' = (1 - z) n + z prev
__global__ __launch_bounds__(256) void roland_gru_kernel(const float* __restrict__ gi, const float* __restrict__ gh, const float* __restrict__ prev,
                                                         long long ldp, int C, long long N, float* __restrict__ out) {
  const long long total = N * C;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += step) {
    const long long i = p / C;
    const int c = (int)(p - i * C);
    const float* a = gi + i * 3 * C + c;
    const float* b = gh + i * 3 * C + c;
    const float r = 1.f / (1.f + expf(-(a[0] + b[0])));
    const float z = 1.f / (1.f + expf(-(a[C] + b[C])));
    const float n = tanhf(a[2 * C] + r * b[2 * C]);
    out[p] = (1.f - z) * n + z * prev[i * ldp + c];
  }
}

}  // namespace tgmx

using namespace tgmx;

extern "C" size_t tgmx_gcn_workspace_bytes(int64_t E, int64_t N) {
  GcnWorkspace w;
  if (E < 0 || E >= (1ll << 31) || N <= 0 || N >= (1ll << 31)) return 0;
  return gcn_carve(nullptr, E, N, w) == TGMX_OK ? w.total : 0;
}

extern "C" int tgmx_gcn_norm_csr(const void* src, const void* dst, int32_t idx64, const float* w, int64_t E, int64_t N, float fill,
                                 int32_t add_self_loops, int32_t* indptr, int32_t* cols, float* vals, float* diag, void* workspace,
                                 size_t workspace_bytes, int32_t* skipped, tgmx_stream_t stream) {
  TGMX_REQUIRE(E >= 0 && E < (1ll << 31) && N > 0 && N < (1ll << 31), "gcn_norm_csr: bad sizes E=%lld N=%lld", (long long)E, (long long)N);
  TGMX_REQUIRE(indptr && diag && workspace && (E == 0 || (src && dst && cols && vals)), "gcn_norm_csr: null pointer");
  hipStream_t st = (hipStream_t)stream;
  GcnWorkspace l;
  if (gcn_carve(workspace, E, N, l) != TGMX_OK || workspace_bytes < l.total) {
    set_error("gcn_norm_csr: workspace too small (%zu bytes)", workspace_bytes);
    return TGMX_E_INVALID;
  }
  const int cb = col_bits(N);
  const float* we = E > 0 ? w : nullptr;
  if (add_self_loops && hipMemsetAsync(l.loop_e, 0xff, (size_t)N * sizeof(int), st) != hipSuccess) {  // -1: no explicit self loop
    set_error("gcn_norm_csr: clearing the self-loop slots failed");
    return TGMX_E_LAUNCH;
  }
  if (E > 0) {  // (a zero-length sort is not issued)
    hipLaunchKernelGGL(gcn_keys_kernel, dim3(grid_for(E, 256, 4096)), dim3(256), 0, st, src, dst, idx64, (long long)E, (long long)N, cb,
                       add_self_loops ? 1 : 0, l.kd_in, l.pos_in, l.loop_e, skipped);
    TGMX_CHECK_LAUNCH("gcn_norm_csr(keys)");
    if (sort_keys_pos(l.temp, l.temp_bytes, l.kd_in, l.kd_out, l.pos_in, l.pos_out, (size_t)E, cb, st) != hipSuccess) {
      set_error("gcn_norm_csr: radix sort failed");
      return TGMX_E_LAUNCH;
    }
  }
  hipLaunchKernelGGL(gcn_node_kernel, dim3(grid_for(N, kSpmmWaves, 4096)), dim3(kSpmmThreads), 0, st, l.kd_out, l.pos_out, we, l.loop_e, (long long)E,
                     (long long)N, cb, fill, add_self_loops ? 1 : 0, indptr, l.dinv, diag);
  TGMX_CHECK_LAUNCH("gcn_norm_csr(nodes)");
  if (E > 0) {
    hipLaunchKernelGGL(gcn_entries_kernel, dim3(grid_for(E, 256, 4096)), dim3(256), 0, st, l.kd_out, l.pos_out, we, l.dinv, (long long)E, cb, cols, vals);
    TGMX_CHECK_LAUNCH("gcn_norm_csr(entries)");
  }
  return TGMX_OK;
}

extern "C" int tgmx_gcn_propagate(const int32_t* indptr, const int32_t* cols, const float* vals, const float* diag, int64_t N, int32_t C,
                                  const float* t, int64_t ldt, const float* bias, int32_t epilogue, const float* prev, int64_t ldp, float tau,
                                  const float* tau_ptr, float* prev_copy, int64_t ldc, float* out, int64_t ldo, int64_t nnz, float* scratch,
                                  size_t scratch_floats, tgmx_stream_t stream) {
  const bool blend = epilogue == TGMX_GCN_EPI_TAU;
  TGMX_REQUIRE(epilogue >= TGMX_GCN_EPI_NONE && epilogue <= TGMX_GCN_EPI_TAU, "gcn_propagate: unknown epilogue %d", epilogue);
  TGMX_REQUIRE(N >= 0 && N < (1ll << 31) && C > 0 && ldt >= C && ldo >= C && (!blend || ldp >= C) && (!blend || !prev_copy || ldc >= C) && nnz >= 0 &&
                   nnz < (1ll << 31),
               "gcn_propagate: bad sizes N=%lld C=%d nnz=%lld", (long long)N, C, (long long)nnz);
  if (N == 0) return TGMX_OK;
  TGMX_REQUIRE(indptr && diag && t && out && (!blend || prev) && (nnz == 0 || (cols && vals)), "gcn_propagate: null pointer");
  float* copy = blend ? prev_copy : nullptr;
  SpmmArgs<GcnEpi> a{indptr, cols, vals, diag, (long long)N, C, t, (long long)ldt, out, (long long)ldo, 0, nullptr,
                     GcnEpi{bias, epilogue, blend ? prev : nullptr, (long long)ldp, tau, blend ? tau_ptr : nullptr, copy, (long long)ldc}};
  const bool vec = spmm_vec_ok(t, ldt) && spmm_vec_ok(out, ldo) && (!bias || spmm_vec_ok(bias, 4)) && (!blend || spmm_vec_ok(prev, ldp)) &&
                   (!copy || spmm_vec_ok(copy, ldc));
  return spmm_run(a, nnz, scratch, scratch_floats, vec, "gcn_propagate", (hipStream_t)stream);
}

extern "C" int tgmx_roland_forward(const tgmx_roland_fwd_t* a, tgmx_stream_t stream) {
  TGMX_REQUIRE(a, "roland_forward: null argument block");
  const int64_t N = a->N;
  const int C = a->C, in = a->in_ch, up = a->update;
  TGMX_REQUIRE(N > 0 && N < (1ll << 31) && C > 0 && C < (1 << 28) && in > 0 && a->E >= 0, "roland_forward: bad sizes");
  TGMX_REQUIRE(up >= TGMX_ROLAND_TAU && up <= TGMX_ROLAND_GRU, "roland_forward: unknown update %d", up);
  TGMX_REQUIRE(a->x && a->xw && a->out[0] && a->out[1] && a->conv_w[0] && a->conv_w[1] && a->ldw[0] >= in && a->ldw[1] >= C,
               "roland_forward: null pointer or narrow weights");
  if (up == TGMX_ROLAND_TAU) TGMX_REQUIRE(a->prev[0] && a->prev[1] && a->ldp >= C, "roland_forward: the tau update needs prev");
  else TGMX_REQUIRE(a->op[0] && a->op[1], "roland_forward: the mlp / gru update needs its operands");
  if (up == TGMX_ROLAND_MLP) TGMX_REQUIRE(a->mlp_w[0] && a->mlp_w[1], "roland_forward: the mlp update needs its weights");
  if (up == TGMX_ROLAND_GRU)
    TGMX_REQUIRE(a->w_ih[0] && a->w_ih[1] && a->w_hh[0] && a->w_hh[1] && a->gi && a->gh, "roland_forward: the gru update needs its weights and gi / gh");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if ((rc = tgmx_gcn_norm_csr(a->src, a->dst, a->idx64, nullptr, a->E, N, a->fill, a->add_self_loops, a->indptr, a->cols, a->vals, a->diag, a->norm_ws,
                              a->norm_ws_bytes, a->skipped, stream)))
    return rc;
  for (int l = 0; l < 2; ++l) {
    const float* h_in = l == 0 ? a->x : a->out[0];
    const int kin = l == 0 ? in : C;
    if ((rc = tgmx_sgemm_nt(h_in, kin, a->conv_w[l], a->ldw[l], a->xw, C, N, C, kin, nullptr, 0, 1, 0, 0, 0, stream))) return rc;
    if (up == TGMX_ROLAND_TAU) {
      if ((rc = tgmx_gcn_propagate(a->indptr, a->cols, a->vals, a->diag, N, C, a->xw, C, a->conv_b[l], TGMX_GCN_EPI_TAU, a->prev[l], a->ldp, a->tau,
                                   a->tau_ptr, a->prev_copy[l], C, a->out[l], C, a->E, a->prop_ws, a->prop_ws_floats, stream)))
        return rc;
      continue;
    }
    float* op = a->op[l];  // [relu(conv_l) | prev_l]
    if ((rc = tgmx_gcn_propagate(a->indptr, a->cols, a->vals, a->diag, N, C, a->xw, C, a->conv_b[l], TGMX_GCN_EPI_RELU, nullptr, 0, 0.f, nullptr, nullptr,
                                 0, op, 2 * C, a->E, a->prop_ws, a->prop_ws_floats, stream)))
      return rc;
    if (up == TGMX_ROLAND_MLP) {
      if ((rc = tgmx_sgemm_nt(op, 2 * C, a->mlp_w[l], 2 * C, a->out[l], C, N, C, 2 * C, a->mlp_b[l], 0, 1, 0, 0, 0, stream))) return rc;
    } else {
      if ((rc = tgmx_sgemm_nt(op, 2 * C, a->w_ih[l], C, a->gi, 3 * C, N, 3 * C, C, a->b_ih[l], 0, 1, 0, 0, 0, stream))) return rc;
      if ((rc = tgmx_sgemm_nt(op + C, 2 * C, a->w_hh[l], C, a->gh, 3 * C, N, 3 * C, C, a->b_hh[l], 0, 1, 0, 0, 0, stream))) return rc;
      hipLaunchKernelGGL(roland_gru_kernel, dim3(grid_for(N * C, 256, 16384)), dim3(256), 0, st, a->gi, a->gh, op + C, (long long)2 * C, C, (long long)N,
                         a->out[l]);
      TGMX_CHECK_LAUNCH("roland_forward(gru)");
    }
  }
  return TGMX_OK;
}
