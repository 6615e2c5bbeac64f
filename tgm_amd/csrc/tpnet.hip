// TPNet (the reference's tgm/nn/encoder/tpnet.py) for gfx950: the streaming temporal walk matrices as random projections (decay +
// deterministic scatter-add per batch), the pair features (small Gram matrices over gathered table rows), the token-matrix assembly of the
// encoder, the token mean, and the inference forward as one call.  The dense contractions (the pair-feature MLP, the two projections,
// the channel FFNs) run on the exact-fp32 MFMA GEMM of csrc/dense.hip through tgmx_sgemm_nt_ep; token mixing is csrc/mixer.hip's block with a
// corrected column mean (tgmx_tpnet_token_mix).
#include "common.h"

namespace tgmx {

constexpr int kHeadEmpty = TGMX_TPNET_HEAD_EMPTY;
constexpr int kTpThreads = 256;
constexpr int kTpWaves = kTpThreads / kWave;

// ---- update ---------------------------------------------------------------------------------------------------------------------------
// The batch's 2 n contributions in the reference's order: j < n is edge j seen from its source (target src[j], message from dst[j]),
// j >= n is edge j - n seen from its destination.  Level m + 1 receives messages read from level m.
//
// Launch 1 (stage) only READS the tables: msg[m][j][:] = (P[m][other_j] * decay^m) * w_j for every level, i.e. the value the reference
// reads after its rescale and before any scatter of this batch.  It also records, per target row, the first contribution that names it
// (an integer atomicMin: the outcome does not depend on the order of arrival).
// Launch 2 (apply) gives every table element to one lane: P[i][r][c] *= decay^i, then the staged messages of row r are added in
// contribution order (the target list is scanned once per row).  A row without a message is left alone when decay is exactly 1.  No float atomics, no element written by two threads: two runs from one state give the same bits.

struct UpdateArgs {
  tgmx_tpnet_tables_t tb;
  const int32_t* src;
  const int32_t* dst;
  const int64_t* time;
  long long n;
  double lambda;
  const void* now;
  int now_is_f64;
  float* msg;
  int32_t* head;
};

__device__ __forceinline__ double since_now(const UpdateArgs& a) {
  const long long next = a.time[a.n - 1];
  return a.now_is_f64 ? (double)next - *reinterpret_cast<const double*>(a.now) : (double)(next - *reinterpret_cast<const int64_t*>(a.now));
}

__device__ __forceinline__ int target_of(const UpdateArgs& a, long long j) { return j < a.n ? a.src[j] : a.dst[j - a.n]; }
__device__ __forceinline__ int other_of(const UpdateArgs& a, long long j) { return j < a.n ? a.dst[j] : a.src[j - a.n]; }

__global__ __launch_bounds__(kTpThreads) void tpnet_stage_kernel(UpdateArgs a) {
  const int lane = lane_id();
  const long long wave = (long long)blockIdx.x * kTpWaves + threadIdx.x / kWave;
  const long long nwaves = (long long)gridDim.x * kTpWaves;
  const int L = a.tb.levels - 1, dim = a.tb.dim;
  const long long N = a.tb.num_nodes, n2 = 2 * a.n;
  const long long next = a.time[a.n - 1];
  const double dnow = since_now(a);
  for (long long it = wave; it < n2 * L; it += nwaves) {
    const int m = (int)(it / n2);
    const long long j = it - (long long)m * n2;
    const long long e = j < a.n ? j : j - a.n;
    const int tgt = target_of(a, j), oth = other_of(a, j);
    const bool ok = tgt >= 0 && tgt < N && oth >= 0 && oth < N;
    const float w = (float)exp(-a.lambda * (double)(next - a.time[e]));
    const float sc = m ? (float)exp(-a.lambda * dnow * (double)m) : 1.f;
    const float* __restrict__ row = a.tb.P[m] + (long long)(ok ? oth : 0) * dim;
    float* __restrict__ o = a.msg + it * dim;
    for (int c = lane; c < dim; c += kWave) o[c] = ok ? (row[c] * sc) * w : 0.f;
    if (m == 0 && lane == 0 && ok) atomicMin(&a.head[tgt], (int)j);
  }
}

__global__ __launch_bounds__(kTpThreads) void tpnet_apply_kernel(UpdateArgs a) {
  const int lane = lane_id();
  const long long wave = (long long)blockIdx.x * kTpWaves + threadIdx.x / kWave;
  const long long nwaves = (long long)gridDim.x * kTpWaves;
  const int L = a.tb.levels - 1, dim = a.tb.dim;
  const long long N = a.tb.num_nodes, n2 = 2 * a.n;
  const double dnow = since_now(a);
  for (long long r = wave; r < N; r += nwaves) {
    const int h = a.head[r];
    if (h == kHeadEmpty && dnow == 0.0) continue;  // decay is exactly 1 and nothing arrives: the row keeps its bits
    // every element of the row belongs to one lane for the whole call: rescale it, then add its messages through memory, in order
    for (int i = 1; i <= L; ++i) {
      const float sc = (float)exp(-a.lambda * dnow * (double)i);
      float* row = a.tb.P[i] + r * dim;
      for (int c = lane; c < dim; c += kWave) row[c] = row[c] * sc;
    }
    if (h == kHeadEmpty) continue;
    // ONE scan of the batch's target list per row, from the first contribution that names it
    for (long long j0 = h & ~(long long)(kWave - 1); j0 < n2; j0 += kWave) {
      const long long jj = j0 + lane;
      const bool mine = jj >= h && jj < n2 && target_of(a, jj) == (int)r;
      unsigned long long hits = __ballot(mine);
      while (hits) {
        const int b = __ffsll((long long)hits) - 1;
        hits &= hits - 1;
        for (int i = 1; i <= L; ++i) {
          float* row = a.tb.P[i] + r * dim;
          const float* msg = a.msg + ((long long)(i - 1) * n2 + j0 + b) * dim;
          for (int c = lane; c < dim; c += kWave) row[c] += msg[c];
        }
      }
    }
    if (lane == 0) a.head[r] = kHeadEmpty;  // only this wave reads head[r]
  }
}

// ---- pair features -----------------------------------------------------------------------------------------------------------------------
// One wave per item.  The lanes split the dim columns of the 2 (L + 1) gathered rows (VEC floats per lane and step), every lane keeps
// the partial sums of the Gram entries in registers, a butterfly over the wave finishes them, and lane r NR + s stores entry (r, s).
// The stacked rows [item, 2 L + 2, dim] never exist in memory.

__device__ __forceinline__ long long wrap_row(int id, long long N) {
  long long r = id < 0 ? (long long)id + N : (long long)id;  // torch indexing: -1 (PADDED_NODE_ID) is the last row
  return r < 0 ? 0 : (r >= N ? N - 1 : r);
}

template <int NL, bool CONCAT, int VEC>
__global__ __launch_bounds__(kTpThreads) void tpnet_pair_kernel(tgmx_tpnet_tables_t tb, const int32_t* __restrict__ a, const int32_t* __restrict__ a_rows,
                                                               long long a_num_rows, int k, const int32_t* __restrict__ b0,
                                                               const int32_t* __restrict__ b1, long long bmod, long long n, int scale,
                                                               float* __restrict__ out, long long ldo) {
  constexpr int NR = CONCAT ? 2 * NL : NL;  // rows / columns of the result
  constexpr int OUT = NR * NR;
  static_assert(OUT <= kWave, "one lane per entry");
  const int lane = lane_id();
  const long long wave = (long long)blockIdx.x * kTpWaves + threadIdx.x / kWave;
  const long long nwaves = (long long)gridDim.x * kTpWaves;
  const long long total = b1 ? 2 * n : n;
  const int dim = tb.dim;
  for (long long item = wave; item < total; item += nwaves) {
    const bool second = item >= n;
    const long long t = second ? item - n : item;
    const long long q = t / k;
    const int j = (int)(t - q * k);
    const long long hr = a_rows ? (long long)a_rows[q] : q;
    const int ida = (hr >= 0 && hr < a_num_rows) ? a[hr * k + j] : -1;
    const int idb = (second ? b1 : b0)[q % bmod];
    const long long ra = wrap_row(ida, tb.num_nodes) * dim, rb = wrap_row(idb, tb.num_nodes) * dim;
    float acc[NR][NR];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int s = 0; s < NR; ++s) acc[r][s] = 0.f;
    for (int c = lane * VEC; c < dim; c += kWave * VEC) {
      float va[NL][VEC], vb[NL][VEC];
#pragma unroll
      for (int l = 0; l < NL; ++l) {
        if constexpr (VEC == 2) {
          const float2 x = *reinterpret_cast<const float2*>(tb.P[l] + ra + c);
          const float2 y = *reinterpret_cast<const float2*>(tb.P[l] + rb + c);
          va[l][0] = x.x, va[l][1] = x.y, vb[l][0] = y.x, vb[l][1] = y.y;
        } else {
          va[l][0] = tb.P[l][ra + c];
          vb[l][0] = tb.P[l][rb + c];
        }
      }
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        if constexpr (CONCAT) {
#pragma unroll
          for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int s = r; s < NR; ++s)
              acc[r][s] = __fmaf_rn(r < NL ? va[r][v] : vb[r - NL][v], s < NL ? va[s][v] : vb[s - NL][v], acc[r][s]);
        } else {
#pragma unroll
          for (int r = 0; r < NL; ++r)
#pragma unroll
            for (int s = 0; s < NL; ++s) acc[r][s] = __fmaf_rn(va[r][v], vb[s][v], acc[r][s]);
        }
      }
    }
    float val = 0.f;
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int s = CONCAT ? r : 0; s < NR; ++s) {
        float x = acc[r][s];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
        if (lane == r * NR + s || (CONCAT && lane == s * NR + r)) val = x;
      }
    if (scale) val = log1pf(val < 0.f ? 0.f : val);  // clamp the negatives, then log(x + 1)
    float* __restrict__ o = out + item * ldo;
    if (lane < OUT) o[lane] = val;
    for (long long c = OUT + lane; c < ldo; c += kWave) o[c] = 0.f;
  }
}

template <int NL, bool CONCAT>
static void launch_pair(bool vec2, unsigned blocks, hipStream_t st, const tgmx_tpnet_tables_t& tb, const int32_t* a, const int32_t* a_rows,
                        long long a_num_rows, int k, const int32_t* b0, const int32_t* b1, long long bmod, long long n, int scale, float* out,
                        long long ldo) {
  if (vec2)
    hipLaunchKernelGGL((tpnet_pair_kernel<NL, CONCAT, 2>), dim3(blocks), dim3(kTpThreads), 0, st, tb, a, a_rows, a_num_rows, k, b0, b1, bmod, n, scale, out, ldo);
  else
    hipLaunchKernelGGL((tpnet_pair_kernel<NL, CONCAT, 1>), dim3(blocks), dim3(kTpThreads), 0, st, tb, a, a_rows, a_num_rows, k, b0, b1, bmod, n, scale, out, ldo);
}

// ---- token matrix -------------------------------------------------------------------------------------------------------------------------
// one wave per token row (q, j): [node_x[id] | cos(w log(dt + 1) + b) | edge features | pair block 0 | pair block 1 | 0 pad]
__global__ __launch_bounds__(kTpThreads) void tpnet_tokens_kernel(const float* __restrict__ node_x, long long num_nodes, int dN,
                                                                 const int64_t* __restrict__ edge_time, long long B,
                                                                 const int32_t* __restrict__ nids, const int64_t* __restrict__ nbr_t,
                                                                 const float* __restrict__ nbr_x, long long S, int k, int dE,
                                                                 const int32_t* __restrict__ rows,
                                                                 const float* __restrict__ tw, const float* __restrict__ tbias, int dT,
                                                                 const float* __restrict__ pf, long long ldpf, int pfd, float* __restrict__ out,
                                                                 long long ldo, double* __restrict__ lg_out) {
  const int lane = lane_id();
  const long long wave = (long long)blockIdx.x * kTpWaves + threadIdx.x / kWave;
  const long long nwaves = (long long)gridDim.x * kTpWaves;
  const long long R = 2 * B * k;
  for (long long row = wave; row < R; row += nwaves) {
    const long long q = row / k;
    const int j = (int)(row - q * k);
    const long long p = q < B ? q : q - B;
    const long long hr = rows ? (long long)rows[q] : q;
    const bool inb = hr >= 0 && hr < S;
    const long long slot = (inb ? hr : 0) * k + j;
    const int id = inb ? nids[slot] : -1;
    const bool pad = id == -1;
    const bool has_x = !pad && id >= 0 && id < num_nodes;
    // the reference takes log of the int64 gap + 1 and feeds Time2Vec; here in double up to the cosine, rounded once
    const double lg = pad ? 0.0 : log((double)(edge_time[p] - nbr_t[slot] + 1));
    if (lg_out && lane == 0) lg_out[row] = pad ? -1.0 : lg;  // (training: what the time encoder's backward needs of the caller's tensors)
    float* __restrict__ o = out + row * ldo;
    for (int c = lane; c < dN; c += kWave) o[c] = has_x ? node_x[(long long)id * dN + c] : 0.f;
    for (int c = lane; c < dT; c += kWave) o[dN + c] = pad ? 0.f : (float)cos(fma((double)tw[c], lg, (double)tbias[c]));
    for (int c = lane; c < dE; c += kWave) o[dN + dT + c] = inb ? nbr_x[slot * dE + c] : 0.f;
    const int base = dN + dT + dE;
    for (int c = lane; c < 2 * pfd; c += kWave) {
      const int blk = c >= pfd;
      o[base + c] = pf[((long long)blk * R + row) * ldpf + (c - blk * pfd)];
    }
    for (long long c = base + 2 * pfd + lane; c < ldo; c += kWave) o[c] = 0.f;
  }
}

// out[q, c] = mean over the k token rows of sequence q
__global__ __launch_bounds__(256) void tpnet_mean_kernel(const float* __restrict__ z, long long ldz, long long Q, int k, int C, float* __restrict__ out,
                                                        long long ldo) {
  const long long total = Q * C;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
    const long long q = e / C;
    const int c = (int)(e - q * C);
    const float* __restrict__ zs = z + q * k * ldz + c;
    float a = 0.f;
#pragma unroll 8
    for (int j = 0; j < k; ++j) a += zs[j * ldz];
    out[q * ldo + c] = a / (float)k;
  }
}

static bool tables_ok(const tgmx_tpnet_tables_t* tb) {
  if (!tb || tb->levels < 1 || tb->levels > TGMX_TPNET_MAX_LEVELS || tb->dim < 1 || tb->num_nodes < 1) return false;
  for (int i = 0; i < tb->levels; ++i)
    if (!tb->P[i]) return false;
  return true;
}

static unsigned wave_blocks(long long items) {
  long long blocks = (items + kTpWaves - 1) / kTpWaves;
  return (unsigned)(blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks));
}

}  // namespace tgmx

using namespace tgmx;

extern "C" int tgmx_tpnet_update(const tgmx_tpnet_tables_t* tables, const int32_t* src, const int32_t* dst, const int64_t* time, int64_t n,
                                 double lambda, const void* now, int32_t now_is_f64, int64_t* now_out, float* msg, int32_t* head,
                                 tgmx_stream_t stream) {
  TGMX_REQUIRE(tables_ok(tables), "tpnet_update: bad tables (1 .. %d levels, dim > 0, num_nodes > 0, no null table)", TGMX_TPNET_MAX_LEVELS);
  TGMX_REQUIRE(n >= 0 && 2 * n < (long long)TGMX_TPNET_HEAD_EMPTY, "tpnet_update: n=%lld: contribution indices 0 .. 2 n - 1 must stay below the empty mark %d",
               (long long)n, TGMX_TPNET_HEAD_EMPTY);
  if (n == 0) return TGMX_OK;
  TGMX_REQUIRE(src && dst && time && now && now_out && head && (tables->levels == 1 || msg), "tpnet_update: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (tables->levels > 1) {
    UpdateArgs a{*tables, src, dst, time, (long long)n, lambda, now, now_is_f64, msg, head};
    hipLaunchKernelGGL(tpnet_stage_kernel, dim3(wave_blocks(2 * n * (tables->levels - 1))), dim3(kTpThreads), 0, st, a);
    TGMX_CHECK_LAUNCH("tpnet_update(stage)");
    hipLaunchKernelGGL(tpnet_apply_kernel, dim3(wave_blocks(tables->num_nodes)), dim3(kTpThreads), 0, st, a);
    TGMX_CHECK_LAUNCH("tpnet_update(apply)");
  }
  if (hipMemcpyAsync(now_out, time + (n - 1), sizeof(int64_t), hipMemcpyDeviceToDevice, st) != hipSuccess) {
    set_error("tpnet_update: copying the batch's last time failed");
    return TGMX_E_LAUNCH;
  }
  return TGMX_OK;
}

extern "C" int tgmx_tpnet_pair_features(const tgmx_tpnet_tables_t* tables, const int32_t* a, const int32_t* a_rows, int64_t a_num_rows,
                                        int32_t k, const int32_t* b0, const int32_t* b1, int64_t bmod, int64_t n, int32_t concat,
                                        int32_t scale, float* out, int64_t ldo, tgmx_stream_t stream) {
  TGMX_REQUIRE(tables_ok(tables), "tpnet_pair_features: bad tables (1 .. %d levels, dim > 0, num_nodes > 0, no null table)", TGMX_TPNET_MAX_LEVELS);
  const int NL = tables->levels, NR = concat ? 2 * NL : NL;
  TGMX_REQUIRE(n >= 0 && k > 0 && n % k == 0 && bmod > 0 && a_num_rows >= 0 && ldo >= (int64_t)NR * NR, "tpnet_pair_features: bad sizes n=%lld k=%d ldo=%lld",
               (long long)n, k, (long long)ldo);
  if (n == 0) return TGMX_OK;
  TGMX_REQUIRE(a && b0 && out, "tpnet_pair_features: null pointer");
  if (NL > 4) {
    set_error("tpnet_pair_features: %d tables per side, the kernel keeps the Gram entries of at most 4 in registers", NL);
    return TGMX_E_UNSUPPORTED;
  }
  bool vec2 = tables->dim % 2 == 0;
  for (int i = 0; i < NL; ++i) vec2 = vec2 && ((uintptr_t)tables->P[i] & 7) == 0;
  const unsigned blocks = wave_blocks(b1 ? 2 * n : n);
  hipStream_t st = (hipStream_t)stream;
#define TGMX_PAIR_CASE(L_)                                                                                                       \
  case L_:                                                                                                                       \
    if (concat) launch_pair<L_, true>(vec2, blocks, st, *tables, a, a_rows, a_num_rows, k, b0, b1, bmod, n, scale, out, ldo);   \
    else launch_pair<L_, false>(vec2, blocks, st, *tables, a, a_rows, a_num_rows, k, b0, b1, bmod, n, scale, out, ldo);         \
    break;
  switch (NL) {
    TGMX_PAIR_CASE(1)
    TGMX_PAIR_CASE(2)
    TGMX_PAIR_CASE(3)
    TGMX_PAIR_CASE(4)
  }
#undef TGMX_PAIR_CASE
  TGMX_CHECK_LAUNCH("tpnet_pair_features");
  return TGMX_OK;
}

static int tokens_run(const float* node_x, int64_t num_nodes, int32_t dN, const int64_t* edge_time, int64_t B, const int32_t* nbr_nids,
                      const int64_t* nbr_t, const float* nbr_x, int64_t S, int32_t k, int32_t dE, const int32_t* rows, const float* tw, const float* tb,
                      int32_t dT, const float* pf, int64_t ldpf, int32_t pf_dim, float* out, int64_t ldo, double* lg_out, tgmx_stream_t stream) {
  TGMX_REQUIRE(B >= 0 && S >= 0 && k > 0 && dN >= 0 && dE >= 0 && dT >= 0 && pf_dim >= 0 && num_nodes >= 0 && ldpf >= pf_dim &&
                   ldo >= (int64_t)dN + dT + dE + 2 * pf_dim,
               "tpnet_tokens: bad sizes B=%lld k=%d dN=%d dT=%d dE=%d pf_dim=%d ldo=%lld", (long long)B, k, dN, dT, dE, pf_dim, (long long)ldo);
  if (B == 0) return TGMX_OK;
  TGMX_REQUIRE(rows || S >= 2 * B, "tpnet_tokens: without row indices hop 0 must hold 2 B rows");
  TGMX_REQUIRE(edge_time && nbr_nids && nbr_t && out && (dN == 0 || node_x) && (dE == 0 || nbr_x) && (dT == 0 || (tw && tb)) && (pf_dim == 0 || pf),
               "tpnet_tokens: null pointer");
  hipLaunchKernelGGL(tpnet_tokens_kernel, dim3(wave_blocks(2 * B * k)), dim3(kTpThreads), 0, (hipStream_t)stream, node_x, (long long)num_nodes, dN,
                     edge_time, (long long)B, nbr_nids, nbr_t, nbr_x, (long long)S, k, dE, rows, tw, tb, dT, pf, (long long)ldpf, pf_dim,
                     out, (long long)ldo, lg_out);
  TGMX_CHECK_LAUNCH("tpnet_tokens");
  return TGMX_OK;
}

extern "C" int tgmx_tpnet_tokens(const float* node_x, int64_t num_nodes, int32_t dN, const int64_t* edge_time, int64_t B,
                                 const int32_t* nbr_nids, const int64_t* nbr_t, const float* nbr_x, int64_t S, int32_t k, int32_t dE,
                                 const int32_t* rows, const float* tw, const float* tb, int32_t dT, const float* pf, int64_t ldpf, int32_t pf_dim, float* out, int64_t ldo, tgmx_stream_t stream) {
  return tokens_run(node_x, num_nodes, dN, edge_time, B, nbr_nids, nbr_t, nbr_x, S, k, dE, rows, tw, tb, dT, pf, ldpf, pf_dim, out, ldo, nullptr, stream);
}

extern "C" int tgmx_tpnet_mean(const float* z, int64_t ldz, int64_t Q, int32_t k, int32_t C, float* out, int64_t ldo, tgmx_stream_t stream) {
  TGMX_REQUIRE(Q >= 0 && k > 0 && C > 0 && ldz >= C && ldo >= C, "tpnet_mean: bad sizes Q=%lld k=%d C=%d", (long long)Q, k, C);
  if (Q == 0) return TGMX_OK;
  TGMX_REQUIRE(z && out, "tpnet_mean: null pointer");
  long long blocks = (Q * C + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(tpnet_mean_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z, (long long)ldz, (long long)Q, k, C, out, (long long)ldo);
  TGMX_CHECK_LAUNCH("tpnet_mean");
  return TGMX_OK;
}

// save (training, NULL = inference): layer l reads save->z + l R ldz and keeps its token block's output in save->z1 + l R ldz, the token rows'
// lg go to save->lg -- the same launches in the same order as the inference call, writing elsewhere; drop: the sites' common descriptor.
static int tpnet_forward_run(const tgmx_tpnet_fwd_t* a, const tgmx_tpnet_save_t* save, const tgmx_dropout_t* drop, tgmx_stream_t stream) {
  TGMX_REQUIRE(a && a->num_layers >= 0 && a->num_layers <= TGMX_MIXER_MAX_LAYERS && a->B >= 0 && a->k > 0, "tpnet_forward: bad argument block");
  TGMX_REQUIRE(a->ldf % 4 == 0 && a->ldfh % 4 == 0 && a->ldx0 % 4 == 0 && a->ldhp % 4 == 0 && a->ldz % 4 == 0 && a->ldh % 4 == 0,
               "tpnet_forward: leading dimensions must be multiples of 4");
  const long long B = a->B, Q = 2 * B, R = Q * a->k;
  if (B == 0) return TGMX_OK;
  const int od = a->tables.levels > 0 ? a->rp_out_dim : 0;
  const int W = a->dN + a->dT + a->dE + 2 * od, E = a->E;
  int rc;
  if (od > 0) {
    const int NR = a->rp_concat ? 2 * a->tables.levels : a->tables.levels;
    TGMX_REQUIRE(od == NR * NR, "tpnet_forward: rp_out_dim=%d does not belong to %d tables", od, a->tables.levels);
    // block 0: (neighbour, the edge's source), block 1: (neighbour, the edge's destination)
    if ((rc = tgmx_tpnet_pair_features(&a->tables, a->nbr_nids, a->rows, a->S, a->k, a->src, a->dst, B, R, a->rp_concat, a->rp_scale, a->feat, a->ldf, stream)))
      return rc;
    if ((rc = tgmx_sgemm_nt_ep(a->feat, a->ldf, a->rp_w1, od, a->feat_h, a->ldfh, 2 * R, 4 * od, od, a->rp_b1, 1, nullptr, 0, stream))) return rc;
    if ((rc = tgmx_sgemm_nt_ep(a->feat_h, a->ldfh, a->rp_w2, 4 * od, a->pf, a->ldf, 2 * R, od, 4 * od, a->rp_b2, 0, nullptr, 0, stream))) return rc;
  }
  if ((rc = tokens_run(a->node_x, a->num_nodes, a->dN, a->edge_time, B, a->nbr_nids, a->nbr_t, a->nbr_x, a->S, a->k, a->dE, a->rows, a->tw, a->tb,
                       a->dT, od ? a->pf : nullptr, a->ldf, od, a->x0, a->ldx0, save ? save->lg : nullptr, stream)))
    return rc;
  if ((rc = tgmx_sgemm_nt_ep(a->x0, a->ldx0, a->proj_w0, W, a->hp, a->ldhp, R, 2 * E, W, a->proj_b0, 1, nullptr, 0, stream))) return rc;
  // (the reference's masked_fill after the projection discards its result: pad tokens stay as projected)
  float* z_in = save && a->num_layers > 0 ? save->z : a->z;
  if ((rc = tgmx_sgemm_nt_ep(a->hp, a->ldhp, a->proj_w2, 2 * E, z_in, a->ldz, R, E, 2 * E, a->proj_b2, 0, nullptr, 0, stream))) return rc;
  if (!save) {
    if ((rc = mixer_layers_run(true, a->layers, a->num_layers, Q, a->k, E, a->eps, a->z, a->z1, a->y, a->ldz, a->h, a->ldh, stream))) return rc;
  } else if ((rc = mixer_layers_run_train(true, a->layers, a->num_layers, Q, a->k, E, a->eps, save->z, save->z1, a->z, a->y, a->ldz, a->h, a->ldh, drop,
                                          stream))) {
    return rc;
  }
  return tgmx_tpnet_mean(a->z, a->ldz, Q, a->k, E, a->out, E, stream);
}

extern "C" int tgmx_tpnet_forward(const tgmx_tpnet_fwd_t* a, tgmx_stream_t stream) { return tpnet_forward_run(a, nullptr, nullptr, stream); }

extern "C" int tgmx_tpnet_forward_train(const tgmx_tpnet_fwd_t* a, const tgmx_tpnet_save_t* save, const tgmx_dropout_t* drop, tgmx_stream_t stream) {
  TGMX_REQUIRE(a && save, "tpnet_forward_train: null argument block");
  TGMX_REQUIRE(a->B <= 0 || (save->lg && (a->num_layers <= 0 || (save->z && save->z1))), "tpnet_forward_train: the saving buffers are missing");
  TGMX_REQUIRE(!drop || (drop->p >= 0.f && drop->p < 1.f), "tpnet_forward_train: p must be in [0, 1)");
  for (int l = 0; l < a->num_layers && l < TGMX_MIXER_MAX_LAYERS; ++l)
    if (a->B > 0 && !tgmx_tpnet_train_supported(a->k, a->E, a->layers[l].tok_hidden)) {
      set_error("tpnet_forward_train: layer %d's token block (k=%d, E=%d, hidden %d) is outside the token kernels' envelope", l, a->k, a->E,
                a->layers[l].tok_hidden);
      return TGMX_E_UNSUPPORTED;
    }
  return tpnet_forward_run(a, save, drop, stream);
}
