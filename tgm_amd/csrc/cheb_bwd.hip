// The backward of the GCLSTM cell and of ChebConv (cheb.hip holds the forward and both Laplacian builders) for gfx950: the gate backward, the
// two-addend propagation the reverse Chebyshev recurrence runs on, and the cell's whole backward as one call.
//
// Gate backward: I, F, T, O, C' and tanh(C') are recomputed from pre and Cprev with gclstm_gates_kernel's own expressions (nothing but pre
// is kept of them), then
//   dCn = dC' + dH' O (1 - tanh^2 C'),  dpre_i = dCn T I (1 - I),  dpre_f = dCn Cprev F (1 - F),  dpre_c = dCn I (1 - T^2),
//   dpre_o = dH' tanh(C') O (1 - O),  dCprev = dCn F.
//
// Reverse recurrence: with Tx_0 = H, Tx_1 = L Tx_0, Tx_k = 2 L Tx_{k-1} - Tx_{k-2} and g_k the gradient at Tx_k, Clenshaw's form
//   b_K = b_{K+1} = 0,  b_k = g_k + 2 L^T b_{k+1} - b_{k+2}  (k = K - 1 .. 1),  dH = g_0 + L^T b_1 - b_2
// needs K - 1 propagations over the transpose and no separate axpy: every step is out = alpha (L^T t) + beta prev + gamma prev2 with
// prev = out (b_k overwrites g_k in its own columns).  L^T comes from tgmx_cheb_laplacian_t: no float atomics anywhere, the same bits on
// every run.
#include "common.h"
#include "edge_csr.h"
#include "spmm.h"

namespace tgmx {

// ---- gates --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gclstm_gate_backward_kernel(const float* __restrict__ pre, const float* __restrict__ Cprev, int C, long long N,
                                                                   const float* __restrict__ dH, long long lddh, const float* __restrict__ dC,
                                                                   long long lddc, float* __restrict__ dpre, float* __restrict__ dCprev) {
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
    const float cp = Cprev[p];
    const float cn = F * cp + I * T;
    const float tc = tanhf(cn);
    const float gh = dH ? dH[i * lddh + c] : 0.f;
    const float gc = dC ? dC[i * lddc + c] : 0.f;
    const float dcn = gc + gh * O * (1.f - tc * tc);
    float* d = dpre + i * 4 * C + c;
    d[0] = dcn * T * I * (1.f - I);
    d[C] = dcn * cp * F * (1.f - F);
    d[2 * C] = dcn * I * (1.f - T * T);
    d[3 * C] = gh * tc * O * (1.f - O);
    if (dCprev) dCprev[p] = dcn * F;
  }
}

// ---- propagate with two addends ---------------------------------------------------------------------------------------------------------
// the epilogue of a Clenshaw step over the shared gather SpMM (spmm.h): out = alpha (M t) + beta prev + gamma prev2.  prev may be out itself:
// a lane loads exactly the elements of row i it stores afterwards, in every route (short row, wave 0 of a long row, the join kernel).
struct Cheb2Epi {
  const float* prev;
  const float* prev2;
  long long ldp, ldp2;
  float alpha, beta, gamma;
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
    if (gamma != 0.f) {
      float p[kSpmmChPerLane];
      spmm_load<VEC>(prev2 + i * ldp2, c0, C, lane, p);
#pragma unroll
      for (int q = 0; q < kSpmmChPerLane; ++q) o[q] = __fmaf_rn(gamma, p[q], o[q]);
    }
  }
};

}  // namespace tgmx

using namespace tgmx;

static long long up4ll(long long n) { return (n + 3) / 4 * 4; }

extern "C" int tgmx_gclstm_gate_backward(const float* pre, const float* Cprev, int64_t N, int32_t C, const float* dH_out, int64_t lddh,
                                         const float* dC_out, int64_t lddc, float* dpre, float* dCprev, tgmx_stream_t stream) {
  TGMX_REQUIRE(N >= 0 && N < (1ll << 31) && C > 0 && (!dH_out || lddh >= C) && (!dC_out || lddc >= C), "gclstm_gate_backward: bad sizes N=%lld C=%d",
               (long long)N, C);
  if (N == 0) return TGMX_OK;
  TGMX_REQUIRE(pre && Cprev && dpre, "gclstm_gate_backward: null pointer");
  hipLaunchKernelGGL(gclstm_gate_backward_kernel, dim3(grid_for(N * C, 256, 16384)), dim3(256), 0, (hipStream_t)stream, pre, Cprev, C, (long long)N,
                     dH_out, (long long)lddh, dC_out, (long long)lddc, dpre, dCprev);
  TGMX_CHECK_LAUNCH("gclstm_gate_backward");
  return TGMX_OK;
}

extern "C" int tgmx_cheb_propagate2(const int32_t* indptr, const int32_t* cols, const float* vals, const float* diag, int64_t N, int32_t C,
                                    const float* t, int64_t ldt, const float* prev, int64_t ldp, const float* prev2, int64_t ldp2, float alpha,
                                    float beta, float gamma, float* out, int64_t ldo, int64_t nnz, float* scratch, size_t scratch_floats,
                                    tgmx_stream_t stream) {
  TGMX_REQUIRE(N >= 0 && N < (1ll << 31) && C > 0 && ldt >= C && ldo >= C && (beta == 0.f || ldp >= C) && (gamma == 0.f || ldp2 >= C) && nnz >= 0 &&
                   nnz < (1ll << 31),
               "cheb_propagate2: bad sizes N=%lld C=%d nnz=%lld", (long long)N, C, (long long)nnz);
  if (N == 0) return TGMX_OK;
  TGMX_REQUIRE(indptr && diag && t && out && t != out && (beta == 0.f || prev) && (gamma == 0.f || prev2), "cheb_propagate2: null pointer, or t is out");
  SpmmArgs<Cheb2Epi> a{indptr, cols, vals, diag, (long long)N, C, t, (long long)ldt, out, (long long)ldo, 0, nullptr,
                       Cheb2Epi{prev, prev2, (long long)ldp, (long long)ldp2, alpha, beta, gamma}};
  const bool vec = spmm_vec_ok(t, ldt) && spmm_vec_ok(out, ldo) && (beta == 0.f || spmm_vec_ok(prev, ldp)) && (gamma == 0.f || spmm_vec_ok(prev2, ldp2));
  return spmm_run(a, nnz, scratch, scratch_floats, vec, "cheb_propagate2", (hipStream_t)stream);
}

// dH = g_0 + L^T b_1 - b_2 by Clenshaw's recurrence, in place in g [N, ldg >= K C] (g_k in the columns [k C, (k + 1) C)), K >= 2
extern "C" int tgmx_cheb_clenshaw(const int32_t* indptr, const int32_t* cols, const float* vals, const float* diag, int64_t N, int32_t C, int32_t K,
                                  float* g, int64_t ldg, float* out, int64_t ldo, int64_t nnz, float* scratch, size_t scratch_floats,
                                  tgmx_stream_t stream) {
  TGMX_REQUIRE(K >= 2 && C > 0 && ldg >= (long long)K * C, "cheb_clenshaw: bad sizes K=%d C=%d", K, C);
  TGMX_REQUIRE(g && out, "cheb_clenshaw: null pointer");
  int rc;
  for (int k = K - 2; k >= 1; --k) {  // b_k = g_k + 2 L^T b_{k+1} - b_{k+2}, written over g_k;  b_{K-1} = g_{K-1} as it stands
    float* bk = g + (long long)k * C;
    const bool two = k + 2 < K;
    if ((rc = tgmx_cheb_propagate2(indptr, cols, vals, diag, N, C, bk + C, ldg, bk, ldg, two ? bk + 2 * C : nullptr, ldg, 2.f, 1.f, two ? -1.f : 0.f, bk,
                                   ldg, nnz, scratch, scratch_floats, stream)))
      return rc;
  }
  const bool two = K > 2;
  return tgmx_cheb_propagate2(indptr, cols, vals, diag, N, C, g + C, ldg, g, ldg, two ? g + 2 * C : nullptr, ldg, 1.f, 1.f, two ? -1.f : 0.f, out, ldo, nnz,
                              scratch, scratch_floats, stream);
}

// ---- the cell's backward as one call ------------------------------------------------------------------------------------------------------
static int gclstm_bwd_check(const tgmx_gclstm_bwd_t* a, const char* what) {
  TGMX_REQUIRE(a, "%s: null argument block", what);
  TGMX_REQUIRE(a->N > 0 && a->N < (1ll << 31) && a->C > 0 && a->K > 0 && a->in_ch > 0 && a->E >= 0 && a->E < (1ll << 31), "%s: bad sizes", what);
  const long long width = (long long)a->in_ch + (long long)a->K * a->C;
  TGMX_REQUIRE(width < (1ll << 31) && a->ldop >= width, "%s: operand narrower than in_ch + K C", what);
  TGMX_REQUIRE(!(a->d_x || a->d_H) || (a->WT && a->ldwt >= 4ll * a->C), "%s: a data gradient needs the transposed stacked weight", what);
  TGMX_REQUIRE((!a->dH_out || a->lddh >= a->C) && (!a->dC_out || a->lddc >= a->C), "%s: leading dimension of an upstream gradient", what);
  return TGMX_OK;
}

// dry: walk the workspace only (*need = its size)
static int gclstm_backward_pass(const tgmx_gclstm_bwd_t* a, bool dry, size_t* need, tgmx_stream_t stream) {
  const int64_t N = a->N;
  const int C = a->C, K = a->K, in = a->in_ch;
  const bool graph = a->d_H && K > 1;
  WorkspaceCarver ws(dry ? nullptr : a->workspace);
  int rc;
#define RUN(call)                   \
  do {                              \
    if (!dry && (rc = (call))) return rc; \
  } while (0)
  float* dpre = ws.take<float>((size_t)N * 4 * C);
  // 1. the gates
  RUN(tgmx_gclstm_gate_backward(a->pre, a->Cprev, N, C, a->dH_out, a->lddh, a->dC_out, a->lddc, dpre, a->d_Cprev, stream));
  // 2. the parameters, each in its own layout: d W_g = x^T dpre_g [4, in, C];  d lins_g,k = dpre_g^T Tx_k [K, 4, C, C];  the biases
  if (a->d_W) {
    float* part = ws.take<float>(tgmx_sgemm_tn_workspace_bytes(N, in, C, 4) / sizeof(float));
    RUN(tgmx_sgemm_tn(a->op, a->ldop, dpre, 4 * C, a->d_W, C, N, in, C, 4, 0, C, (int64_t)in * C, 0, part, stream));
  }
  if (a->d_lins) {
    float* part = ws.take<float>(tgmx_sgemm_tn_workspace_bytes(N, 4 * C, C, K) / sizeof(float));
    RUN(tgmx_sgemm_tn(dpre, 4 * C, a->op + in, a->ldop, a->d_lins, C, N, 4 * C, C, K, 0, C, 4ll * C * C, 0, part, stream));
  }
  if (a->d_b || a->d_conv_bias) {
    float* part = ws.take<float>((size_t)256 * 4 * C);
    float* first = a->d_b ? a->d_b : a->d_conv_bias;
    RUN(tgmx_colsum(dpre, 4 * C, N, 4 * C, first, 0, part, stream));
    if (a->d_b && a->d_conv_bias) RUN(tgmx_add_cols(a->d_conv_bias, 4 * C, a->d_b, 4 * C, 1, 4 * C, 0, stream));  // (a copy: the same sums)
  }
  // 3. dop = dpre Wstack, only the columns a requested gradient needs
  if (a->d_x) RUN(tgmx_sgemm_nt(dpre, 4 * C, a->WT, a->ldwt, a->d_x, in, N, in, 4 * C, nullptr, 0, 1, 0, 0, 0, stream));
  if (a->d_H && K == 1) RUN(tgmx_sgemm_nt(dpre, 4 * C, a->WT + (long long)in * a->ldwt, a->ldwt, a->d_H, C, N, C, 4 * C, nullptr, 0, 1, 0, 0, 0, stream));
  if (graph) {
    const long long ldg = up4ll((long long)K * C);
    float* g = ws.take<float>((size_t)N * ldg);
    RUN(tgmx_sgemm_nt(dpre, 4 * C, a->WT + (long long)in * a->ldwt, a->ldwt, g, ldg, N, K * C, 4 * C, nullptr, 0, 1, 0, 0, 0, stream));
    // 4. the reverse recurrence over L^T
    const size_t E = (size_t)a->E, e1 = E > 0 ? E : 1;
    int32_t* indptr = ws.take<int32_t>((size_t)N + 1);
    int32_t* cols = ws.take<int32_t>(e1);
    float* vals = ws.take<float>(e1);
    float* diag = ws.take<float>((size_t)N);
    const size_t lap_bytes = tgmx_cheb_workspace_bytes(a->E, N);
    TGMX_REQUIRE(lap_bytes > 0, "gclstm_backward: %lld edges over %lld nodes are out of range", (long long)a->E, (long long)N);
    char* lap_ws = ws.take<char>(lap_bytes);
    const size_t prop_floats = tgmx_cheb_propagate_scratch_floats(a->E, C);
    float* prop = ws.take<float>(prop_floats);
    RUN(tgmx_cheb_laplacian_t(a->src, a->dst, a->idx64, a->edge_w, a->E, N, a->normalization, a->lambda_max, a->lambda_ptr, indptr, cols, vals, diag,
                              lap_ws, lap_bytes, nullptr, stream));
    RUN(tgmx_cheb_clenshaw(indptr, cols, vals, diag, N, C, K, g, ldg, a->d_H, C, a->E, prop_floats ? prop : nullptr, prop_floats, stream));
  }
#undef RUN
  *need = ws.total();
  return TGMX_OK;
}

extern "C" size_t tgmx_gclstm_backward_workspace_bytes(const tgmx_gclstm_bwd_t* a) {
  size_t need = 0;
  if (gclstm_bwd_check(a, "gclstm_backward_workspace_bytes") != TGMX_OK) return 0;
  return gclstm_backward_pass(a, true, &need, nullptr) == TGMX_OK ? need : 0;
}

extern "C" int tgmx_gclstm_backward(const tgmx_gclstm_bwd_t* a, tgmx_stream_t stream) {
  int rc;
  if ((rc = gclstm_bwd_check(a, "gclstm_backward"))) return rc;
  TGMX_REQUIRE(a->op && a->pre && a->Cprev, "gclstm_backward: the forward's saved buffers are missing");
  TGMX_REQUIRE(!(a->d_H && a->K > 1) || a->E == 0 || (a->src && a->dst), "gclstm_backward: dH over K > 1 needs the edge list");
  size_t need = 0;
  if ((rc = gclstm_backward_pass(a, true, &need, nullptr))) return rc;
  TGMX_REQUIRE(a->workspace && a->workspace_bytes >= need, "gclstm_backward: workspace too small (%zu bytes, %zu needed)", a->workspace_bytes, need);
  return gclstm_backward_pass(a, false, &need, stream);
}
