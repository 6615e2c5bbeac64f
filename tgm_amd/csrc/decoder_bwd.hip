// Training of the decoders (decoder.hip's heads): the forward that keeps every activation the backward reads, and the backward as ONE call.
//
// The backward composes, from the back: the last layer's own kernel when it is at most 16 wide (decoder_tail_bwd: dx, dW and db in one
// pass over the rows), the hidden Linear + ReLU layers from the shared blocks (tgmx_sgemm_tn, tgmx_colsum, tgmx_sgemm_nt on a transposed
// weight, tgmx_relu_mask), and the merge stage.  In the table form the gradient of P [N', 2H] is a scatter of the pair rows; it is read
// back through an inverted index instead (edge_csr.h's sorted keys, spmm.h's gather with unit values): a table row's pairs add in
// ascending pair position, long rows and hubs in spmm.h's fixed splits.  No float atomics: two runs give the same bits.
#include "common.h"
#include "edge_csr.h"
#include "spmm.h"

namespace tgmx {

constexpr int kDecBwdThreads = 256;
constexpr int kDecBwdMaxTail = 16;     // decoder.hip's kDecMaxTail
constexpr int kTailBwdMaxBlocks = 256; // row blocks of the tail backward: the length of the second launch's chain

// ---- the last layer -------------------------------------------------------------------------------------------------------------------------
// Workgroup (bx, by): rows [bx rpb, bx rpb + rpb), columns 64 by + lane of K + 1 (column K is the bias: its "activation" is 1).  Wave w takes
// rows w, w + 4, ... of the block; a lane keeps its column of W and its O partial sums in registers.  The waves' sums meet in LDS in wave
// order; partial [blocks, O, K + 1].
__global__ __launch_bounds__(kDecBwdThreads) void decoder_tail_bwd_kernel(const float* __restrict__ dout, long long lddout,
                                                                          const float* __restrict__ x, long long ldx, long long R, int K,
                                                                          const float* __restrict__ W, int O, int relu, float* __restrict__ dx,
                                                                          long long lddx, float* __restrict__ partial, int rpb) {
  __shared__ float s_part[kDecBwdThreads / kWave - 1][kDecBwdMaxTail][kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int j = blockIdx.y * kWave + lane;
  const bool wcol = j < K, bcol = j == K;
  const long long r0 = (long long)blockIdx.x * rpb, r1 = min(R, r0 + rpb);
  float w[kDecBwdMaxTail], acc[kDecBwdMaxTail];
#pragma unroll
  for (int o = 0; o < kDecBwdMaxTail; ++o) {
    w[o] = (o < O && wcol) ? W[(long long)o * K + j] : 0.f;
    acc[o] = 0.f;
  }
  for (long long r = r0 + wave; r < r1; r += kDecBwdThreads / kWave) {
    const float* __restrict__ dr = dout + r * lddout;
    const float h = wcol ? x[r * ldx + j] : 1.f;
    float s = 0.f;
#pragma unroll
    for (int o = 0; o < kDecBwdMaxTail; ++o) {
      if (o < O) {
        const float d = dr[o];
        s = __fmaf_rn(d, w[o], s);
        acc[o] = __fmaf_rn(d, h, acc[o]);
      }
    }
    if (dx && wcol) dx[r * lddx + j] = (relu && !(h > 0.f)) ? 0.f : s;
  }
  if (!partial) return;  // (the same for every thread)
  if (wave > 0) {
#pragma unroll
    for (int o = 0; o < kDecBwdMaxTail; ++o)
      if (o < O) s_part[wave - 1][o][lane] = acc[o];
  }
  __syncthreads();
  if (wave == 0 && (wcol || bcol)) {
#pragma unroll
    for (int o = 0; o < kDecBwdMaxTail; ++o) {
      if (o < O) {
        float v = acc[o];
#pragma unroll
        for (int u = 0; u < kDecBwdThreads / kWave - 1; ++u) v = __fadd_rn(v, s_part[u][o][lane]);
        partial[((long long)blockIdx.x * O + o) * (K + 1) + j] = v;
      }
    }
  }
}

// dW[o, j], db[o] = the blocks' partials in ascending block order
__global__ __launch_bounds__(kDecBwdThreads) void decoder_tail_bwd_reduce_kernel(const float* __restrict__ partial, int blocks, int O, int K,
                                                                                 float* __restrict__ dW, float* __restrict__ db) {
  const int e = blockIdx.x * kDecBwdThreads + threadIdx.x, OK1 = O * (K + 1);
  if (e >= OK1) return;
  float acc = 0.f;
  for (int b = 0; b < blocks; b += 8) {  // eight loads in flight; the order stays 0, 1, 2, ...
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = b + u < blocks ? partial[(long long)(b + u) * OK1 + e] : 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = __fadd_rn(acc, v[u]);
  }
  const int o = e / (K + 1), j = e - o * (K + 1);
  if (j < K) {
    if (dW) dW[(long long)o * K + j] = acc;
  } else if (db) {
    db[o] = acc;
  }
}

// rows per workgroup: 4 (a row per wave) while that leaves at most kTailBwdMaxBlocks blocks, then what keeps their number there
static int tail_bwd_rpb(long long R) {
  const int waves = kDecBwdThreads / kWave;
  long long rpb = (R + kTailBwdMaxBlocks - 1) / kTailBwdMaxBlocks;
  rpb = (rpb + waves - 1) / waves * waves;
  return (int)(rpb < waves ? waves : rpb);
}

// ---- rows of dropped pairs --------------------------------------------------------------------------------------------------------------------
struct DropJobs {
  tgmx_drop_job_t job[TGMX_DECODER_MAX_LAYERS + 1];
};
// blockIdx.y = job; a thread per element of the job's [R, C]
__global__ __launch_bounds__(kDecBwdThreads) void decoder_drop_rows_kernel(const void* __restrict__ ia, const void* __restrict__ ib, int is64,
                                                                           long long NP, long long R, const DropJobs J) {
  const tgmx_drop_job_t j = J.job[blockIdx.y];
  const long long total = R * j.C, step = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
    const long long r = e / j.C;
    const int c = (int)(e - r * j.C);
    const long long a = ld_idx(ia, is64, r), b = ld_idx(ib, is64, r);
    const bool ok = a >= 0 && a < NP && b >= 0 && b < NP;
    if (!ok) j.dst[r * j.ldd + c] = 0.f;
    else if (j.src) j.dst[r * j.ldd + c] = j.src[r * j.lds + c];
  }
}

// ---- the scatter, as a gather -------------------------------------------------------------------------------------------------------------------
// key t < R: (ia[t] << cb | t), the left half's row ia[t];  key R + t: ((NP + ib[t]) << cb | t), the right half's.  The column is the pair's
// position: the sorted keys ARE the inverted index, a row's pairs in ascending position.
__global__ __launch_bounds__(256) void decoder_scatter_keys_kernel(const void* __restrict__ ia, const void* __restrict__ ib, int is64, long long R,
                                                                   long long NP, int cb, unsigned long long* __restrict__ keys) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < 2 * R; t += step) {
    const long long r = t < R ? t : t - R;
    const long long a = ld_idx(ia, is64, r), b = ld_idx(ib, is64, r);
    const bool ok = a >= 0 && a < NP && b >= 0 && b < NP;
    keys[t] = key_of(ok, t < R ? a : NP + b, r, cb);
  }
}

// row i < NP of the gather is dP[i, :H], row NP + i is dP[i, H:]
struct HalfRowEpi {
  static constexpr bool kGatherOnly = true;
  long long NP;
  int H;
  __device__ __forceinline__ float* row(float* out, long long ldo, long long i) const { return i < NP ? out + i * ldo : out + (i - NP) * ldo + H; }
};

struct ScatterWorkspace {
  unsigned long long *k_in, *k_out;
  char* temp;
  size_t temp_bytes;
  int32_t *indptr, *cols;
  float* chunks;
  size_t chunk_floats, total;
};
static int scatter_carve(void* workspace, long long R, long long NP, int H, ScatterWorkspace& w) {
  WorkspaceCarver c(workspace);
  const size_t n = (size_t)(R > 0 ? 2 * R : 1);
  w.k_in = c.take<unsigned long long>(n);
  w.k_out = c.take<unsigned long long>(n);
  w.temp_bytes = 0;
  if (rocprim::radix_sort_keys(nullptr, w.temp_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, n, 0u, 64u) != hipSuccess)
    return TGMX_E_LAUNCH;
  w.temp = c.take<char>(w.temp_bytes);
  w.indptr = c.take<int32_t>((size_t)(2 * NP + 1));
  w.cols = c.take<int32_t>(n);
  w.chunk_floats = spmm_scratch_floats(2 * R, H);
  w.chunks = c.take<float>(w.chunk_floats);
  w.total = c.total();
  return TGMX_OK;
}

static bool tail_route(const tgmx_decoder_layer_t& ly) { return ly.out <= kDecBwdMaxTail && (int64_t)ly.out * ly.in * sizeof(float) <= 48 * 1024; }

}  // namespace tgmx

using namespace tgmx;

extern "C" size_t tgmx_decoder_tail_bwd_workspace_floats(int64_t R, int32_t K, int32_t out_dim) {
  if (R <= 0 || K <= 0 || out_dim <= 0) return 0;
  const int rpb = tail_bwd_rpb(R);
  return (size_t)((R + rpb - 1) / rpb) * (size_t)out_dim * (size_t)(K + 1);
}

extern "C" int tgmx_decoder_tail_bwd(const float* dout, int64_t lddout, const float* x, int64_t ldx, int64_t R, int32_t K, const float* W,
                                     int32_t out_dim, int32_t relu, float* dx, int64_t lddx, float* dW, float* db, float* workspace,
                                     size_t workspace_floats, tgmx_stream_t stream) {
  if (out_dim <= 0 || out_dim > kDecBwdMaxTail) {
    set_error("decoder_tail_bwd: out_dim=%d (at most %d) outside the kernel's envelope", out_dim, kDecBwdMaxTail);
    return TGMX_E_UNSUPPORTED;
  }
  TGMX_REQUIRE(R >= 0 && R < (1ll << 31) && K > 0 && K < (1 << 24) && lddout >= out_dim && ldx >= K && (!dx || lddx >= K),
               "decoder_tail_bwd: bad sizes R=%lld K=%d", (long long)R, K);
  if (R == 0) return TGMX_OK;
  TGMX_REQUIRE(dout && x && W, "decoder_tail_bwd: null pointer");
  const bool sums = dW || db;
  if (!sums && !dx) return TGMX_OK;
  const int rpb = tail_bwd_rpb(R);
  const int blocks = (int)((R + rpb - 1) / rpb);
  const size_t need = (size_t)blocks * out_dim * (K + 1);
  TGMX_REQUIRE(!sums || (workspace && workspace_floats >= need), "decoder_tail_bwd: workspace too small (%zu floats, %zu needed)", workspace_floats,
               need);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(decoder_tail_bwd_kernel, dim3((unsigned)blocks, (unsigned)((K + 1 + kWave - 1) / kWave)), dim3(kDecBwdThreads), 0, st, dout,
                     (long long)lddout, x, (long long)ldx, (long long)R, K, W, out_dim, relu ? 1 : 0, dx, (long long)lddx,
                     sums ? workspace : nullptr, rpb);
  TGMX_CHECK_LAUNCH("decoder_tail_bwd");
  if (sums) {
    const int OK1 = out_dim * (K + 1);
    hipLaunchKernelGGL(decoder_tail_bwd_reduce_kernel, dim3((unsigned)((OK1 + kDecBwdThreads - 1) / kDecBwdThreads)), dim3(kDecBwdThreads), 0, st,
                       workspace, blocks, out_dim, K, dW, db);
    TGMX_CHECK_LAUNCH("decoder_tail_bwd(reduce)");
  }
  return TGMX_OK;
}

extern "C" int tgmx_decoder_drop_rows(const void* ia, const void* ib, int32_t idx64, int64_t NP, int64_t R, const tgmx_drop_job_t* jobs,
                                      int32_t n_jobs, tgmx_stream_t stream) {
  TGMX_REQUIRE(R >= 0 && NP >= 0 && n_jobs >= 0 && n_jobs <= TGMX_DECODER_MAX_LAYERS + 1, "decoder_drop_rows: bad sizes R=%lld, %d jobs",
               (long long)R, n_jobs);
  if (R == 0 || n_jobs == 0) return TGMX_OK;
  TGMX_REQUIRE(ia && ib && jobs, "decoder_drop_rows: null pointer");
  DropJobs J{};
  long long most = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const tgmx_drop_job_t& j = jobs[i];
    TGMX_REQUIRE(j.dst && j.C > 0 && j.ldd >= j.C && (!j.src || j.lds >= j.C), "decoder_drop_rows: job %d is malformed", i);
    J.job[i] = j;
    most = R * j.C > most ? R * j.C : most;
  }
  hipLaunchKernelGGL(decoder_drop_rows_kernel, dim3(grid_for(most, kDecBwdThreads, 1024), (unsigned)n_jobs), dim3(kDecBwdThreads), 0,
                     (hipStream_t)stream, ia, ib, idx64 ? 1 : 0, (long long)NP, (long long)R, J);
  TGMX_CHECK_LAUNCH("decoder_drop_rows");
  return TGMX_OK;
}

extern "C" size_t tgmx_decoder_scatter_workspace_bytes(int64_t R, int64_t NP, int32_t H) {
  ScatterWorkspace w;
  if (R < 0 || 2 * R >= (1ll << 31) || NP < 0 || 2 * NP >= (1ll << 31) || H <= 0) return 0;
  return scatter_carve(nullptr, R, NP, H, w) == TGMX_OK ? w.total : 0;
}

extern "C" int tgmx_decoder_scatter(const float* dh, int64_t lddh, int64_t R, int32_t H, const void* ia, const void* ib, int32_t idx64, int64_t NP,
                                    float* dP, void* workspace, size_t workspace_bytes, tgmx_stream_t stream) {
  TGMX_REQUIRE(R >= 0 && 2 * R < (1ll << 31) && NP >= 0 && 2 * NP < (1ll << 31) && H > 0 && lddh >= H, "decoder_scatter: bad sizes R=%lld NP=%lld H=%d",
               (long long)R, (long long)NP, H);
  if (NP == 0) return TGMX_OK;
  TGMX_REQUIRE(dP && workspace && (R == 0 || (dh && ia && ib)), "decoder_scatter: null pointer");
  ScatterWorkspace w;
  if (scatter_carve(workspace, R, NP, H, w) != TGMX_OK || workspace_bytes < w.total) {
    set_error("decoder_scatter: workspace too small (%zu bytes)", workspace_bytes);
    return TGMX_E_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const int cb = col_bits(2 * NP > R ? 2 * NP : R);
  const long long n = 2 * R;
  const unsigned long long* sorted = nullptr;
  if (R > 0) {
    hipLaunchKernelGGL(decoder_scatter_keys_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, st, ia, ib, idx64 ? 1 : 0, (long long)R,
                       (long long)NP, cb, w.k_in);
    TGMX_CHECK_LAUNCH("decoder_scatter(keys)");
    if (rocprim::radix_sort_keys(w.temp, w.temp_bytes, (const unsigned long long*)w.k_in, w.k_out, (size_t)n, 0u, (unsigned)(2 * cb + 1), st) !=
        hipSuccess) {
      set_error("decoder_scatter: radix sort failed");
      return TGMX_E_LAUNCH;
    }
    sorted = w.k_out;
  }
  csr_rows_launch(sorted, n, 2 * (long long)NP, cb, w.indptr, w.cols, NoEntryValue{}, st);
  TGMX_CHECK_LAUNCH("decoder_scatter(rows)");
  SpmmArgs<HalfRowEpi> a{w.indptr, w.cols, nullptr, nullptr, 2 * (long long)NP, H, dh, (long long)lddh, dP, 2 * (long long)H, 0, nullptr,
                         HalfRowEpi{(long long)NP, H}};
  const bool vec = spmm_vec_ok(dh, lddh) && spmm_vec_ok(dP, 4) && H % 4 == 0;
  return spmm_run(a, n, w.chunks, w.chunk_floats, vec, "decoder_scatter(gather)", st);
}

// ---- the saving forward -----------------------------------------------------------------------------------------------------------------------
static int train_check(const tgmx_decoder_train_t* t, const char* who) {
  TGMX_REQUIRE(t, "%s: null argument block", who);
  const tgmx_decoder_fwd_t& a = t->fwd;
  TGMX_REQUIRE(a.num_layers >= 1 && a.num_layers <= TGMX_DECODER_MAX_LAYERS && a.R >= 0 && a.R < (1ll << 31), "%s: %d layers, R=%lld", who, a.num_layers,
               (long long)a.R);
  for (int l = 0; l < a.num_layers; ++l) {
    TGMX_REQUIRE(a.layers[l].w && a.layers[l].in > 0 && a.layers[l].out > 0 && (l == 0 || a.layers[l].in == a.layers[l - 1].out),
                 "%s: layer %d is malformed", who, l);
    TGMX_REQUIRE(l == 0 || t->act[l], "%s: no buffer for the input of layer %d", who, l);
  }
  TGMX_REQUIRE(a.pool == TGMX_DECODER_POOL_NONE, "%s: pooling has no training path", who);
  TGMX_REQUIRE(a.merge_act == TGMX_DECODER_ACT_NONE || a.merge_act == TGMX_DECODER_ACT_RELU, "%s: unknown activation %d", who, a.merge_act);
  switch (a.form) {
    case TGMX_DECODER_ROWS:
      TGMX_REQUIRE(a.a1 && a.D > 0 && a.lda1 >= a.D && a.D == a.layers[0].in, "%s(rows): bad operand", who);
      break;
    case TGMX_DECODER_PAIR:
      TGMX_REQUIRE(a.a1 && a.a2 && a.wa && a.wb && t->act[0] && a.D > 0 && a.H > 0 && a.H == a.layers[0].in && a.lda1 >= a.D && a.lda2 >= a.D &&
                       a.ldwa >= a.D && a.ldwb >= a.D && !a.ia && !a.ib && a.n1 >= a.R && a.n2 >= a.R,
                   "%s(pair): bad operand (the training path takes no indices)", who);
      break;
    case TGMX_DECODER_TABLE:
      TGMX_REQUIRE(a.a1 && a.wa && a.wb && t->act[0] && a.ia && a.ib && a.D > 0 && a.H > 0 && a.H == a.layers[0].in && a.lda1 >= a.D &&
                       a.ldwa >= a.D && a.ldwb >= a.D && a.M == -1 && a.B == a.R && a.n1 >= 0 && 2 * a.n1 < (1ll << 31),
                   "%s(table): bad operand (the training path takes flat pairs)", who);
      break;
    default:
      set_error("%s: unknown form %d", who, a.form);
      return TGMX_E_INVALID;
  }
  return TGMX_OK;
}

extern "C" int tgmx_decoder_forward_save(const tgmx_decoder_train_t* t, tgmx_stream_t stream) {
  int rc;
  if ((rc = train_check(t, "decoder_forward_save"))) return rc;
  const tgmx_decoder_fwd_t& a = t->fwd;
  TGMX_REQUIRE(a.out && (a.form != TGMX_DECODER_TABLE || a.P), "decoder_forward_save: null pointer");
  const int D = a.D, H = a.H, L = a.num_layers;
  const int64_t R = a.R;
  if (R == 0) return TGMX_OK;
  const float* x = a.a1;
  int64_t ldx = a.lda1;
  if (a.form == TGMX_DECODER_PAIR) {
    if ((rc = tgmx_decoder_pair_gemm(a.a1, a.lda1, a.n1, nullptr, a.a2, a.lda2, a.n2, nullptr, a.wa, a.ldwa, D, a.wb, a.ldwb, D, a.mbias, a.merge_act,
                                     t->act[0], H, R, H, a.bad, stream)))
      return rc;
  } else if (a.form == TGMX_DECODER_TABLE) {
    if (a.n1 > 0) {  // (no table rows: every pair is out of range, the score kernel reads nothing)
      if ((rc = tgmx_sgemm_nt(a.a1, a.lda1, a.wa, a.ldwa, a.P, 2 * (int64_t)H, a.n1, H, D, a.mbias, 0, 1, 0, 0, 0, stream))) return rc;
      if ((rc = tgmx_sgemm_nt(a.a1, a.lda1, a.wb, a.ldwb, a.P + H, 2 * (int64_t)H, a.n1, H, D, nullptr, 0, 1, 0, 0, 0, stream))) return rc;
    }
    if ((rc = tgmx_decoder_score(a.P, 2 * (int64_t)H, a.n1, H, a.ia, a.ib, nullptr, a.idx64, nullptr, -1, 0, R, a.merge_act, nullptr, nullptr, 0,
                                 t->act[0], H, a.bad, stream)))
      return rc;
  }
  if (a.form != TGMX_DECODER_ROWS) {
    x = t->act[0];
    ldx = H;
  }
  for (int l = 0; l < L; ++l) {
    const tgmx_decoder_layer_t& ly = a.layers[l];
    if (l == L - 1) {
      if (tail_route(ly)) return tgmx_decoder_tail(x, ldx, R, ly.in, ly.w, ly.b, ly.out, a.out, stream);
      return tgmx_sgemm_nt(x, ldx, ly.w, ly.in, a.out, ly.out, R, ly.out, ly.in, ly.b, 0, 1, 0, 0, 0, stream);
    }
    if ((rc = tgmx_sgemm_nt(x, ldx, ly.w, ly.in, t->act[l + 1], ly.out, R, ly.out, ly.in, ly.b, 1, 1, 0, 0, 0, stream))) return rc;
    x = t->act[l + 1];
    ldx = ly.out;
  }
  return TGMX_OK;
}

// ---- the backward -----------------------------------------------------------------------------------------------------------------------------
// One walk over the backward; dry: only the workspace is laid out (*need = its bytes), nothing is launched
static int decoder_backward_pass(const tgmx_decoder_train_t* t, bool dry, size_t* need, tgmx_stream_t stream) {
  const tgmx_decoder_fwd_t& a = t->fwd;
  const int D = a.D, H = a.H, L = a.num_layers;
  const int64_t R = a.R;
  const bool rows = a.form == TGMX_DECODER_ROWS, table = a.form == TGMX_DECODER_TABLE;
  const int64_t NP = a.n1;
  int rc;
#define RUN(call)                      \
  do {                                 \
    if (!dry && (rc = (call))) return rc; \
  } while (0)
  WorkspaceCarver ws(dry ? nullptr : t->workspace);
  const bool merge_dz = t->d_a1 || (!table && t->d_a2);
  const bool need_dx0 = rows ? t->d_a1 != nullptr : (merge_dz || t->d_wa || t->d_wb || t->d_mbias || t->d_mbias2);
  int widest = 1;
  for (int l = 0; l < L; ++l) widest = a.layers[l].in > widest ? a.layers[l].in : widest;
  float* g[2] = {ws.take<float>((size_t)R * widest), ws.take<float>((size_t)R * widest)};
  const float* dout = t->dout;
  int64_t lddout = t->lddout;
  const int out_dim = a.layers[L - 1].out;

  // the rows of dropped pairs: zeros in a copy of dout and, in place, in every saved activation
  if (table) {
    float* clean = ws.take<float>((size_t)R * out_dim);
    tgmx_drop_job_t jobs[TGMX_DECODER_MAX_LAYERS + 1];
    int n = 0;
    jobs[n++] = tgmx_drop_job_t{dout, clean, lddout, out_dim, out_dim, 0};
    jobs[n++] = tgmx_drop_job_t{nullptr, t->act[0], 0, H, H, 0};
    for (int l = 1; l < L; ++l) jobs[n++] = tgmx_drop_job_t{nullptr, t->act[l], 0, a.layers[l].in, a.layers[l].in, 0};
    RUN(tgmx_decoder_drop_rows(a.ia, a.ib, a.idx64, NP, R, jobs, n, stream));
    dout = clean;
    lddout = out_dim;
  }

  // the weights as the NT GEMMs of the dX steps read them: one launch
  float* wt[TGMX_DECODER_MAX_LAYERS] = {nullptr};
  float* wmt = nullptr;  // [D, 2H]: [Wa^T | Wb^T]
  {
    tgmx_pack_job_t jobs[TGMX_DECODER_MAX_LAYERS + 2];
    int n = 0;
    for (int l = 0; l < L; ++l) {
      const tgmx_decoder_layer_t& ly = a.layers[l];
      if ((l == L - 1 && tail_route(ly)) || !(l > 0 || need_dx0)) continue;
      wt[l] = ws.take<float>((size_t)ly.in * ly.out);
      jobs[n++] = tgmx_pack_job_t{ly.w, wt[l], ly.in, ly.out, ly.in, ly.out, ly.in, ly.out, 1, 0};
    }
    if (!rows && merge_dz) {
      wmt = ws.take<float>((size_t)D * 2 * H);
      jobs[n++] = tgmx_pack_job_t{a.wa, wmt, a.ldwa, 2 * (int64_t)H, D, H, D, H, 1, 0};
      jobs[n++] = tgmx_pack_job_t{a.wb, wmt + H, a.ldwb, 2 * (int64_t)H, D, H, D, H, 1, 0};
    }
    if (n) RUN(tgmx_pack2d(jobs, n, stream));
  }

  const auto tn = [&](const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t rows_, int M, int N) -> int {
    float* part = ws.take<float>(tgmx_sgemm_tn_workspace_bytes(rows_, M, N, 1) / sizeof(float));
    return dry ? TGMX_OK : tgmx_sgemm_tn(A, lda, B, ldb, C, ldc, rows_, M, N, 1, 0, 0, 0, 0, part, stream);
  };
  const auto colsum = [&](const float* X, int64_t ld, int64_t rows_, int C, float* out) -> int {
    float* part = ws.take<float>((size_t)256 * C);
    return dry ? TGMX_OK : tgmx_colsum(X, ld, rows_, C, out, 0, part, stream);
  };

  // the layers, from the back: dY is the gradient of layer l's output before its activation
  const float* dY = dout;
  int64_t lddy = lddout;
  int cur = 0;
  for (int l = L - 1; l >= 0; --l) {
    const tgmx_decoder_layer_t& ly = a.layers[l];
    const float* X = l ? t->act[l] : (rows ? a.a1 : t->act[0]);
    const int64_t ldx = l ? ly.in : (rows ? a.lda1 : H);
    const bool x_relu = l > 0 || (!rows && a.merge_act == TGMX_DECODER_ACT_RELU);
    const bool want_dx = l > 0 || need_dx0;
    float* dX = (l == 0 && rows) ? t->d_a1 : g[cur];
    if (l == L - 1 && tail_route(ly)) {
      const size_t floats = (t->d_w[l] || t->d_b[l]) ? tgmx_decoder_tail_bwd_workspace_floats(R, ly.in, ly.out) : 0;
      float* part = ws.take<float>(floats);
      RUN(tgmx_decoder_tail_bwd(dY, lddy, X, ldx, R, ly.in, ly.w, ly.out, x_relu, want_dx ? dX : nullptr, ly.in, t->d_w[l], t->d_b[l], part, floats,
                                stream));
    } else {
      if (t->d_w[l] && (rc = tn(dY, lddy, X, ldx, t->d_w[l], ly.in, R, ly.out, ly.in))) return rc;
      if (t->d_b[l] && (rc = colsum(dY, lddy, R, ly.out, t->d_b[l]))) return rc;
      if (want_dx) {
        RUN(tgmx_sgemm_nt(dY, lddy, wt[l], ly.out, dX, ly.in, R, ly.in, ly.out, nullptr, 0, 1, 0, 0, 0, stream));
        if (x_relu) RUN(tgmx_relu_mask(dX, ly.in, X, ldx, R, ly.in, stream));
      }
    }
    if (!want_dx) return (*need = ws.total(), TGMX_OK);
    dY = dX;
    lddy = ly.in;
    cur ^= 1;
  }
  if (rows) return (*need = ws.total(), TGMX_OK);

  // the merge stage: dY is dh0 [R, H]
  if (t->d_mbias && (rc = colsum(dY, H, R, H, t->d_mbias))) return rc;
  if (t->d_mbias2 && (rc = colsum(dY, H, R, H, t->d_mbias2))) return rc;
  if (!table) {
    if (t->d_wa && (rc = tn(dY, H, a.a1, a.lda1, t->d_wa, t->ld_dwa, R, H, D))) return rc;
    if (t->d_wb && (rc = tn(dY, H, a.a2, a.lda2, t->d_wb, t->ld_dwb, R, H, D))) return rc;
    if (t->d_a1) RUN(tgmx_sgemm_nt(dY, H, wmt, 2 * (int64_t)H, t->d_a1, D, R, D, H, nullptr, 0, 1, 0, 0, 0, stream));
    if (t->d_a2) RUN(tgmx_sgemm_nt(dY, H, wmt + H, 2 * (int64_t)H, t->d_a2, D, R, D, H, nullptr, 0, 1, 0, 0, 0, stream));
  } else if (NP > 0 && (t->d_wa || t->d_wb || t->d_a1)) {
    float* dP = ws.take<float>((size_t)NP * 2 * H);
    const size_t bytes = tgmx_decoder_scatter_workspace_bytes(R, NP, H);
    char* sws = ws.take<char>(bytes);
    RUN(tgmx_decoder_scatter(dY, H, R, H, a.ia, a.ib, a.idx64, NP, dP, sws, bytes, stream));
    if (t->d_wa && (rc = tn(dP, 2 * (int64_t)H, a.a1, a.lda1, t->d_wa, t->ld_dwa, NP, H, D))) return rc;
    if (t->d_wb && (rc = tn(dP + H, 2 * (int64_t)H, a.a1, a.lda1, t->d_wb, t->ld_dwb, NP, H, D))) return rc;
    if (t->d_a1) RUN(tgmx_sgemm_nt(dP, 2 * (int64_t)H, wmt, 2 * (int64_t)H, t->d_a1, D, NP, D, 2 * H, nullptr, 0, 1, 0, 0, 0, stream));
  }
#undef RUN
  *need = ws.total();
  return TGMX_OK;
}

extern "C" size_t tgmx_decoder_backward_workspace_bytes(const tgmx_decoder_train_t* t) {
  size_t need = 0;
  if (train_check(t, "decoder_backward_workspace_bytes") != TGMX_OK) return 0;
  return decoder_backward_pass(t, true, &need, nullptr) == TGMX_OK ? need : 0;
}

extern "C" int tgmx_decoder_backward(const tgmx_decoder_train_t* t, tgmx_stream_t stream) {
  int rc;
  if ((rc = train_check(t, "decoder_backward"))) return rc;
  const tgmx_decoder_fwd_t& a = t->fwd;
  TGMX_REQUIRE(t->dout && t->lddout >= a.layers[a.num_layers - 1].out, "decoder_backward: no upstream gradient");
  TGMX_REQUIRE((!t->d_wa || t->ld_dwa >= a.D) && (!t->d_wb || t->ld_dwb >= a.D), "decoder_backward: leading dimension of a merge gradient");
  TGMX_REQUIRE(a.form != TGMX_DECODER_ROWS || !(t->d_a2 || t->d_wa || t->d_wb || t->d_mbias || t->d_mbias2), "decoder_backward(rows): no merge stage");
  TGMX_REQUIRE(a.form != TGMX_DECODER_TABLE || !t->d_a2, "decoder_backward(table): one table, one gradient");
  if (a.R == 0) return TGMX_OK;
  size_t need = 0;
  if ((rc = decoder_backward_pass(t, true, &need, nullptr))) return rc;
  TGMX_REQUIRE(t->workspace && t->workspace_bytes >= need, "decoder_backward: workspace too small (%zu bytes, %zu needed)", t->workspace_bytes, need);
  return decoder_backward_pass(t, false, &need, stream);
}
