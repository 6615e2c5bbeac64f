// DyGFormer / TransformerEncoder training: the backward of tgmx_dygformer_forward_train (csrc/dygformer.hip) as one call, and its pieces.
//
//   tgmx_mha_small_backward               the attention backward: one workgroup per (group, head), probabilities recomputed in LDS
//   tgmx_dygformer_mean_backward          the per-side patch mean
//   tgmx_dygformer_time_backward          the Time2Vec channel: per-slot rows whose column sums are d time_encoder.w.*
//   tgmx_dygformer_cooccurrence_backward  the co-occurrence table and its encoder
//   tgmx_dygformer_layer_backward         one transformer layer
//   tgmx_dygformer_backward               the whole chain; GEMMs and reductions are the dense library's (tgmx_sgemm_nt_ep, tgmx_sgemm_tn,
//                                         tgmx_colsum, tgmx_ln_backward, tgmx_add_cols, tgmx_dropout, tgmx_mixer_gelu_backward)
//
// No float atomics anywhere: every sum over rows goes through tgmx_sgemm_tn / tgmx_colsum, whose orders are fixed.
#include <math.h>

#include "common.h"
#include "edge_csr.h"
#include "gemm.h"
#include "mha_small.h"

namespace tgmx {

// ---- attention backward ---------------------------------------------------------------------------------------------------------------------
// LDS: Q, K, V, dO [Tp][ldk] (zero outside T x dh), PM [Tp][ldp] the dropped probabilities, DS [Tp][lds] the score gradients -- all
// resident (mha_small.h).  Phase 1, a wave per 16-row tile i: the scores, max / sum / exp / division exactly as mha_small_kernel takes
// them (same MFMA order, same reductions over the 16 lanes of a group), so P is the forward's, bit for bit; then dP = dO V^T in a second
// set of accumulators with the same lane layout, the mask, delta = rowsum(dP o P) over the 16 lanes, and PM / DS written.  Phase 2: the
// 3 nI nN output tiles (dQ | dK | dV, 16 rows x 16 columns each) dealt round-robin to the four waves; the A operand is DS by rows (dQ),
// DS transposed (dK) or PM transposed (dV), the B operand K / Q / dO by rows of k.  Each output element belongs to one tile: written once.
__global__ __launch_bounds__(256) void mha_small_backward_kernel(const float* __restrict__ qkv, long long ldq, const float* __restrict__ datt,
                                                                 long long ldo, int T, int H, int dh, float scale, float* __restrict__ dqkv,
                                                                 int ldk, int ldp, int lds_, const DropoutArgs drop) {
  extern __shared__ float lds[];
  const int Tp = (T + 15) & ~15, nI = Tp >> 4, dh4 = (dh + 3) & ~3, D = H * dh;
  float* __restrict__ Q = lds;
  float* __restrict__ K = Q + (size_t)Tp * ldk;
  float* __restrict__ V = K + (size_t)Tp * ldk;
  float* __restrict__ DO = V + (size_t)Tp * ldk;
  float* __restrict__ PM = DO + (size_t)Tp * ldk;
  float* __restrict__ DS = PM + (size_t)Tp * ldp;
  const long long grp = blockIdx.x / H;
  const int h = blockIdx.x % H;
  const float* __restrict__ base = qkv + grp * T * ldq + (long long)h * dh;
  const float* __restrict__ dbase = datt + grp * T * ldo + (long long)h * dh;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, lc = lane & 15, lg = lane >> 4;
  for (int e = tid; e < Tp * ldk; e += 256) {
    const int r = e / ldk, c = e - r * ldk;
    const bool ok = r < T && c < dh;
    Q[e] = ok ? base[(long long)r * ldq + c] : 0.f;
    K[e] = ok ? base[(long long)r * ldq + D + c] : 0.f;
    V[e] = ok ? base[(long long)r * ldq + 2 * D + c] : 0.f;
    DO[e] = ok ? dbase[(long long)r * ldo + c] : 0.f;
  }
  __syncthreads();
  for (int i = wave; i < nI; i += 4) {
    floatx4 acc[kMhaJ], dac[kMhaJ];
#pragma unroll
    for (int j = 0; j < kMhaJ; ++j) acc[j] = dac[j] = floatx4{0.f, 0.f, 0.f, 0.f};
    {
      const float* __restrict__ qa = Q + (i * 16 + lc) * ldk + lg;
      const float* __restrict__ kb = K + lc * ldk + lg;
      for (int kk = 0; kk < dh4; kk += 4) {
        const float a = qa[kk];
#pragma unroll
        for (int j = 0; j < kMhaJ; ++j)
          if (j < nI) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, kb[j * 16 * ldk + kk], acc[j], 0, 0, 0);
      }
      const float* __restrict__ da = DO + (i * 16 + lc) * ldk + lg;
      const float* __restrict__ vb = V + lc * ldk + lg;
      for (int kk = 0; kk < dh4; kk += 4) {
        const float a = da[kk];
#pragma unroll
        for (int j = 0; j < kMhaJ; ++j)
          if (j < nI) dac[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, vb[j * 16 * ldk + kk], dac[j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float m = -INFINITY;
#pragma unroll
      for (int j = 0; j < kMhaJ; ++j)
        if (j < nI) {
          acc[j][r] *= scale;
          if (j * 16 + lc < T) m = fmaxf(m, acc[j][r]);
        }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < kMhaJ; ++j)
        if (j < nI) {
          const float ex = j * 16 + lc < T ? expf(acc[j][r] - m) : 0.f;
          acc[j][r] = ex;
          s += ex;
        }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
      const int row = i * 16 + 4 * lg + r;
      const unsigned long long e0 = ((unsigned long long)blockIdx.x * T + row) * T + lc;
      float delta = 0.f;
#pragma unroll
      for (int j = 0; j < kMhaJ; ++j)
        if (j < nI) {
          const bool ok = row < T && j * 16 + lc < T;
          const float p = ok ? acc[j][r] / s : 0.f;  // rows past T carry no gradient
          const float mk = ok ? dropout_scale(drop, e0 + j * 16) : 0.f;
          const float dp = dac[j][r] * mk;
          acc[j][r] = p;
          dac[j][r] = dp;
          delta = __fmaf_rn(dp, p, delta);
          PM[row * ldp + j * 16 + lc] = p * mk;
        }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) delta += __shfl_xor(delta, o);
#pragma unroll
      for (int j = 0; j < kMhaJ; ++j)
        if (j < nI) DS[row * lds_ + j * 16 + lc] = acc[j][r] * (dac[j][r] - delta);
    }
  }
  __syncthreads();
  const int nN = (dh + 15) >> 4, per = nI * nN;
  for (int t = wave; t < 3 * per; t += 4) {
    const int which = t / per, rem = t - which * per, i = rem / nN, n = rem - i * nN;
    const int col = n * 16 + lc;
    const bool cok = col < ldk;  // columns [dh, ldk) hold zeros
    const float* __restrict__ B = (which == 0 ? K : which == 1 ? Q : DO) + lg * ldk + (cok ? col : 0);
    // A[m][k]: dQ reads DS[16 i + m][k]; dK reads DS[k][16 i + m]; dV reads PM[k][16 i + m]
    const float* __restrict__ A = which == 0 ? DS + (i * 16 + lc) * lds_ + lg : which == 1 ? DS + lg * lds_ + i * 16 + lc : PM + lg * ldp + i * 16 + lc;
    const int ak = which == 0 ? 1 : which == 1 ? lds_ : ldp;
    floatx4 o = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < Tp; kk += 4) {
      const float b = cok ? B[kk * ldk] : 0.f;
      o = __builtin_amdgcn_mfma_f32_16x16x4f32(A[kk * ak], b, o, 0, 0, 0);
    }
    const float f = which == 2 ? 1.f : scale;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = i * 16 + 4 * lg + r;
      if (row < T && col < dh) dqkv[(grp * T + row) * ldq + (long long)which * D + (long long)h * dh + col] = o[r] * f;
    }
  }
}

// ---- the small pieces -----------------------------------------------------------------------------------------------------------------------
// one workgroup per sequence q = 2 p + side
__global__ __launch_bounds__(256) void dyg_mean_backward_kernel(const float* __restrict__ dmean, long long ldm, long long P, int Np, int D,
                                                               float* __restrict__ dx, long long ldx) {
  const long long q = blockIdx.x;
  const float* __restrict__ g = dmean + ((q & 1) * P + (q >> 1)) * ldm;
  const int total = Np * D;
  for (int e = threadIdx.x; e < total; e += blockDim.x) {
    const int t = e / D, c = e - t * D;
    dx[(q * Np + t) * ldx + c] = g[c] / (float)Np;
  }
}

struct DygSeqsB {
  const int32_t *src, *dst, *src_rows, *dst_rows;
  long long P, S;
};

// the forward's slot logic (dyg_prologue_kernel): one thread per (slot row, time channel)
__global__ __launch_bounds__(256) void dyg_time_backward_kernel(DygSeqsB sq, const float* __restrict__ dtime, long long ldt,
                                                               const int64_t* __restrict__ edge_time, const int32_t* __restrict__ nbr_nids,
                                                               const int64_t* __restrict__ nbr_t, int k, const float* __restrict__ tw,
                                                               const float* __restrict__ tb, int dT, float* __restrict__ rows) {
  const int L = k + 1;
  const long long total = 2 * sq.P * L * dT;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
    const long long r = e / dT;
    const int ct = (int)(e - r * dT);
    const long long q = r / L;
    const int j = (int)(r - q * L);
    const long long p = q >> 1;
    const bool d = q & 1;
    const int32_t seed = d ? sq.dst[p] : sq.src[p];
    const int32_t* rws = d ? sq.dst_rows : sq.src_rows;
    long long row = rws ? (long long)rws[p] : (d ? sq.P + p : p);
    if (row < 0 || row >= sq.S) row = -1;
    const long long slot = row < 0 ? -1 : row * k + j - 1;
    const int32_t id = j == 0 ? seed : (slot < 0 ? -1 : nbr_nids[slot]);
    float gw = 0.f, gb = 0.f;
    if (id != -1) {
      const float dt = (j == 0 || slot < 0) ? 0.f : (float)(edge_time[p] - nbr_t[slot]);
      gb = -sinf(__fmaf_rn(dt, tw[ct], tb[ct])) * dtime[r * ldt + ct];
      gw = gb * dt;
    }
    rows[r * 2 * dT + ct] = gw;
    rows[r * 2 * dT + dT + ct] = gb;
  }
}

// onehot[r, c] = (own_r == c) + (other_r == c), c < ldh
__global__ __launch_bounds__(256) void dyg_onehot_kernel(const int32_t* __restrict__ counts, long long n, int ldh, float* __restrict__ onehot) {
  const long long total = n * ldh;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
    const long long r = e / ldh;
    const int c = (int)(e - r * ldh);
    onehot[e] = (float)((counts[2 * r] == c) + (counts[2 * r + 1] == c));
  }
}

// r[c, j] = relu(fma(w1[j], c, b1[j])), as dyg_cotable_kernel takes it
__global__ __launch_bounds__(256) void dyg_cohidden_kernel(const float* __restrict__ w1, const float* __restrict__ b1, int C, int ld,
                                                          float* __restrict__ r) {
  const float c = (float)blockIdx.x;
  for (int j = threadIdx.x; j < C; j += blockDim.x) r[(long long)blockIdx.x * ld + j] = fmaxf(__fmaf_rn(w1[j], c, b1[j]), 0.f);
}

// dh[c, j] = r[c, j] > 0 ? dh[c, j] : 0;  dhc[c, j] = dh[c, j] c
__global__ __launch_bounds__(256) void dyg_cohidden_backward_kernel(float* __restrict__ dh, const float* __restrict__ r, int C, int ld,
                                                                   float* __restrict__ dhc) {
  const float c = (float)blockIdx.x;
  for (int j = threadIdx.x; j < C; j += blockDim.x) {
    const long long e = (long long)blockIdx.x * ld + j;
    const float v = r[e] > 0.f ? dh[e] : 0.f;
    dh[e] = v;
    dhc[e] = v * c;
  }
}

static unsigned dyg_blocks(long long total) {
  long long blocks = (total + 255) / 256;
  return (unsigned)(blocks > 16384 ? 16384 : (blocks < 1 ? 1 : blocks));
}

static bool drop_ok(const tgmx_dropout_t* d) { return !d || (d->p >= 0.f && d->p < 1.f); }
static int up4i(long long v) { return (int)((v + 3) / 4 * 4); }

}  // namespace tgmx

using namespace tgmx;

extern "C" int tgmx_mha_small_train_supported(int32_t T, int32_t dh) {
  if (T <= 0 || dh <= 0 || T > kMhaMaxT || dh > kMhaMaxDh) return 0;
  return mha_bwd_lds_bytes(T, dh) <= kMhaMaxLds ? 1 : 0;
}

extern "C" int tgmx_mha_small_backward(const float* qkv, int64_t ldq, const float* datt, int64_t ldo, int64_t B, int32_t T, int32_t H,
                                       int32_t dh, float* dqkv, const tgmx_dropout_t* drop, tgmx_stream_t stream) {
  TGMX_REQUIRE(B >= 0 && T > 0 && H > 0 && dh > 0 && (long long)H * dh < (1 << 28) && ldq >= 3ll * H * dh && ldo >= (long long)H * dh &&
                   B * H < (1ll << 31) && drop_ok(drop),
               "mha_small_backward: bad sizes B=%lld T=%d H=%d dh=%d", (long long)B, T, H, dh);
  if (!tgmx_mha_small_train_supported(T, dh)) {
    set_error("mha_small_backward: T=%d tokens x head dimension %d is outside the training envelope (Q, K, V, dO and two T x T tiles in %zu bytes of LDS)",
              T, dh, kMhaMaxLds);
    return TGMX_E_UNSUPPORTED;
  }
  if (B == 0) return TGMX_OK;
  TGMX_REQUIRE(qkv && datt && dqkv && dqkv != qkv, "mha_small_backward: null or aliased pointer");
  const int Tp = (T + 15) & ~15, ldk = mha_ld((dh + 3) & ~3), ldp = mha_bwd_ld_pm(Tp), lds = mha_bwd_ld_ds(Tp);
  const size_t bytes = mha_bwd_lds_bytes(T, dh);
  if (bytes > 64 * 1024) {  // past the default limit of a launch; set per call: the attribute belongs to the current device
    const hipError_t attr = hipFuncSetAttribute((const void*)mha_small_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMhaMaxLds);
    if (attr != hipSuccess) {
      (void)hipGetLastError();
      set_error("mha_small_backward: T=%d x dh=%d needs %zu bytes of LDS and the limit cannot be raised: %s", T, dh, bytes, hipGetErrorString(attr));
      return TGMX_E_UNSUPPORTED;
    }
  }
  hipLaunchKernelGGL(mha_small_backward_kernel, dim3((unsigned)(B * H)), dim3(256), bytes, (hipStream_t)stream, qkv, (long long)ldq, datt,
                     (long long)ldo, T, H, dh, 1.f / sqrtf((float)dh), dqkv, ldk, ldp, lds, make_dropout(drop));
  TGMX_CHECK_LAUNCH("mha_small_backward");
  return TGMX_OK;
}

extern "C" int tgmx_dygformer_mean_backward(const float* dmean, int64_t ldm, int64_t P, int32_t Np, int32_t D, float* dx, int64_t ldx,
                                            tgmx_stream_t stream) {
  TGMX_REQUIRE(P >= 0 && Np > 0 && D > 0 && ldm >= D && ldx >= D && 2 * P < (1ll << 31) && (long long)Np * D < (1ll << 31),
               "dygformer_mean_backward: bad sizes P=%lld Np=%d D=%d", (long long)P, Np, D);
  if (P == 0) return TGMX_OK;
  TGMX_REQUIRE(dmean && dx, "dygformer_mean_backward: null pointer");
  hipLaunchKernelGGL(dyg_mean_backward_kernel, dim3((unsigned)(2 * P)), dim3(256), 0, (hipStream_t)stream, dmean, (long long)ldm, (long long)P, Np, D, dx,
                     (long long)ldx);
  TGMX_CHECK_LAUNCH("dygformer_mean_backward");
  return TGMX_OK;
}

extern "C" int tgmx_dygformer_time_backward(const float* dtime, int64_t ldt, const int32_t* src, const int32_t* dst, const int64_t* edge_time,
                                            int64_t P, const int32_t* nbr_nids, const int64_t* nbr_t, int64_t S, int32_t k,
                                            const int32_t* src_rows, const int32_t* dst_rows, const float* tw, const float* tb, int32_t dT,
                                            float* rows, tgmx_stream_t stream) {
  TGMX_REQUIRE(P >= 0 && S >= 0 && k >= 0 && k < 2048 && dT > 0 && ldt >= dT, "dygformer_time_backward: bad sizes P=%lld S=%lld k=%d dT=%d",
               (long long)P, (long long)S, k, dT);
  if (P == 0) return TGMX_OK;
  TGMX_REQUIRE(dtime && src && dst && edge_time && (k == 0 || S == 0 || (nbr_nids && nbr_t)) && tw && tb && rows, "dygformer_time_backward: null pointer");
  const DygSeqsB sq{src, dst, src_rows, dst_rows, (long long)P, (long long)S};
  hipLaunchKernelGGL(dyg_time_backward_kernel, dim3(dyg_blocks(2 * P * (k + 1) * dT)), dim3(256), 0, (hipStream_t)stream, sq, dtime, (long long)ldt,
                     edge_time, nbr_nids, nbr_t, k, tw, tb, dT, rows);
  TGMX_CHECK_LAUNCH("dygformer_time_backward");
  return TGMX_OK;
}

// dry: lay the workspace out only
static int co_backward_pass(const int32_t* counts, const float* dfeat, int64_t ldf, int64_t n, int L, int C, const float* w1, const float* b1,
                            const float* w2T, float* d_w1, float* d_b1, float* d_w2, float* d_b2, void* workspace, bool dry, size_t* need,
                            tgmx_stream_t stream) {
  const int ldo = up4i(L + 1), ldc = up4i(C), T = L + 1;
  WorkspaceCarver ws(dry ? nullptr : workspace);
  float* onehot = ws.take<float>((size_t)n * ldo);
  float* dtable = ws.take<float>((size_t)T * ldc);
  float* r = ws.take<float>((size_t)T * ldc);
  float* dh = ws.take<float>((size_t)T * ldc);
  float* dhc = ws.take<float>((size_t)T * ldc);
  size_t tn = tgmx_sgemm_tn_workspace_bytes(n, T, C, 1);
  const size_t tn2 = tgmx_sgemm_tn_workspace_bytes(T, C, C, 1);
  tn = tn2 > tn ? tn2 : tn;
  float* tn_ws = ws.take<float>(tn / sizeof(float) + 1);
  float* cs_ws = ws.take<float>((size_t)256 * C);
  *need = ws.total();
  if (dry) return TGMX_OK;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  hipLaunchKernelGGL(dyg_onehot_kernel, dim3(dyg_blocks(n * ldo)), dim3(256), 0, st, counts, (long long)n, ldo, onehot);
  TGMX_CHECK_LAUNCH("dygformer_cooccurrence_backward(onehot)");
  if ((rc = tgmx_sgemm_tn(onehot, ldo, dfeat, ldf, dtable, ldc, n, T, C, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
  if (d_b2 && (rc = tgmx_colsum(dtable, ldc, T, C, d_b2, 0, cs_ws, stream))) return rc;
  if (!(d_w2 || d_w1 || d_b1)) return TGMX_OK;
  hipLaunchKernelGGL(dyg_cohidden_kernel, dim3((unsigned)T), dim3(C <= 64 ? 64 : 256), 0, st, w1, b1, C, ldc, r);
  TGMX_CHECK_LAUNCH("dygformer_cooccurrence_backward(hidden)");
  if (d_w2 && (rc = tgmx_sgemm_tn(dtable, ldc, r, ldc, d_w2, C, T, C, C, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
  if (!(d_w1 || d_b1)) return TGMX_OK;
  if ((rc = tgmx_sgemm_nt_ep(dtable, ldc, w2T, C, dh, ldc, T, C, C, nullptr, 0, nullptr, 0, stream))) return rc;
  hipLaunchKernelGGL(dyg_cohidden_backward_kernel, dim3((unsigned)T), dim3(C <= 64 ? 64 : 256), 0, st, dh, r, C, ldc, dhc);
  TGMX_CHECK_LAUNCH("dygformer_cooccurrence_backward(relu)");
  if (d_w1 && (rc = tgmx_colsum(dhc, ldc, T, C, d_w1, 0, cs_ws, stream))) return rc;
  if (d_b1 && (rc = tgmx_colsum(dh, ldc, T, C, d_b1, 0, cs_ws, stream))) return rc;
  return TGMX_OK;
}

extern "C" size_t tgmx_dygformer_cooccurrence_backward_workspace_bytes(int64_t n, int32_t L, int32_t C) {
  if (n < 0 || L <= 0 || C <= 0) return 0;
  size_t need = 0;
  co_backward_pass(nullptr, nullptr, 0, n, L, C, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, true, &need, nullptr);
  return need;
}

extern "C" int tgmx_dygformer_cooccurrence_backward(const int32_t* counts, const float* dfeat, int64_t ldf, int64_t n, int32_t L, int32_t C,
                                                    const float* co_w1, const float* co_b1, const float* co_w2T, float* d_w1, float* d_b1,
                                                    float* d_w2, float* d_b2, void* workspace, size_t workspace_bytes, tgmx_stream_t stream) {
  TGMX_REQUIRE(n >= 0 && n < (1ll << 31) && L > 0 && L <= 2048 && C > 0 && ldf >= C, "dygformer_cooccurrence_backward: bad sizes n=%lld L=%d C=%d",
               (long long)n, L, C);
  if (n == 0 || !(d_w1 || d_b1 || d_w2 || d_b2)) return TGMX_OK;
  TGMX_REQUIRE(counts && dfeat && co_w1 && co_b1 && co_w2T, "dygformer_cooccurrence_backward: null pointer");
  size_t need = 0;
  co_backward_pass(nullptr, nullptr, 0, n, L, C, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, true, &need, nullptr);
  TGMX_REQUIRE(workspace && workspace_bytes >= need, "dygformer_cooccurrence_backward: workspace too small (%zu bytes, %zu needed)", workspace_bytes, need);
  return co_backward_pass(counts, dfeat, ldf, n, L, C, co_w1, co_b1, co_w2T, d_w1, d_b1, d_w2, d_b2, workspace, false, &need, stream);
}

// ---- one layer --------------------------------------------------------------------------------------------------------------------------------
static int layer_backward_pass(const tgmx_dygformer_layer_t* ly, const tgmx_dygformer_layer_tr_t* tr, const tgmx_dygformer_layer_grad_t* d, int64_t B,
                               int T, int H, int D, float eps, const float* x, const float* qkv, const float* att, const float* x1, int64_t ldx,
                               int64_t ldq, int64_t ldh, float* g, float* dx, const tgmx_dropout_t* drop, void* workspace, bool dry, size_t* need,
                               tgmx_stream_t stream) {
  const int64_t R = B * T;
  const bool dropping = drop && drop->p > 0.f;
  WorkspaceCarver ws(dry ? nullptr : workspace);
  const size_t Rx = (size_t)R * ldx, Rh = (size_t)R * ldh;
  float* y = ws.take<float>(Rx);
  float* abuf = ws.take<float>(Rh);
  float* hbuf = ws.take<float>(Rh);
  float* dy = ws.take<float>(Rx);
  float* du = ws.take<float>(Rx);
  float* dgx = ws.take<float>(Rx);
  float* gt = ws.take<float>(dropping ? Rx : 0);
  float* datt = ws.take<float>(Rx);
  float* dqkv = ws.take<float>((size_t)R * ldq);
  float* zero = ws.take<float>((size_t)ldx);
  size_t tn = tgmx_sgemm_tn_workspace_bytes(R, D, 4 * D, 1);
  auto grow = [&](size_t b) { tn = b > tn ? b : tn; };
  grow(tgmx_sgemm_tn_workspace_bytes(R, 4 * D, D, 1));
  grow(tgmx_sgemm_tn_workspace_bytes(R, 3 * D, D, 1));
  grow(tgmx_sgemm_tn_workspace_bytes(R, D, D, 1));
  float* tn_ws = ws.take<float>(tn / sizeof(float) + 1);
  float* cs_ws = ws.take<float>((size_t)256 * 4 * D);
  *need = ws.total();
  if (dry) return TGMX_OK;

  hipStream_t st = (hipStream_t)stream;
  tgmx_dropout_t site[4];
  for (int s = 0; s < 4; ++s) site[s] = dropping ? tgmx_dropout_t{drop->p, drop->seed, drop->stream + s, 0} : tgmx_dropout_t{0.f, 0, 0, 0};
  int rc;
  if (hipMemsetAsync(zero, 0, (size_t)ldx * sizeof(float), st) != hipSuccess) {
    set_error("dygformer_layer_backward: hipMemsetAsync failed");
    return TGMX_E_LAUNCH;
  }
  // the FFN
  if ((rc = tgmx_layernorm_rows(x1, ldx, R, D, ly->ln1_g, ly->ln1_b, eps, y, ldx, stream))) return rc;
  if ((rc = tgmx_sgemm_nt_ep(y, ldx, ly->w1, D, abuf, ldh, R, 4 * D, D, ly->b1, 0, nullptr, 0, stream))) return rc;
  const float* g3 = g;
  if (dropping) {
    if ((rc = tgmx_dropout(g, ldx, R, D, &site[3], gt, ldx, stream))) return rc;
    g3 = gt;
  }
  if ((rc = tgmx_sgemm_nt_ep(g3, ldx, tr->w2T, D, hbuf, ldh, R, 4 * D, D, nullptr, 0, nullptr, 0, stream))) return rc;
  if ((rc = tgmx_mixer_gelu_backward(abuf, ldh, hbuf, ldh, R, 4 * D, &site[2], stream))) return rc;
  if (d->w2 && (rc = tgmx_sgemm_tn(g3, ldx, abuf, ldh, d->w2, 4 * D, R, D, 4 * D, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
  if (d->b2 && (rc = tgmx_colsum(g3, ldx, R, D, d->b2, 0, cs_ws, stream))) return rc;
  if (d->w1 && (rc = tgmx_sgemm_tn(hbuf, ldh, y, ldx, d->w1, D, R, 4 * D, D, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
  if (d->b1 && (rc = tgmx_colsum(hbuf, ldh, R, 4 * D, d->b1, 0, cs_ws, stream))) return rc;
  const bool attn = d->ln0_g || d->ln0_b || d->in_w || d->in_b || d->out_w || d->out_b || dx;  // somebody reads dx1
  if (!(d->ln1_g || d->ln1_b || attn)) return TGMX_OK;
  if ((rc = tgmx_sgemm_nt_ep(hbuf, ldh, tr->w1T, 4 * D, dy, ldx, R, D, 4 * D, nullptr, 0, nullptr, 0, stream))) return rc;
  if ((rc = tgmx_ln_backward(dy, ldx, x1, ldx, zero, 0, ly->ln1_g, D, eps, R, du, ldx, dgx, ldx, stream))) return rc;
  if (d->ln1_g && (rc = tgmx_colsum(dgx, ldx, R, D, d->ln1_g, 0, cs_ws, stream))) return rc;
  if (d->ln1_b && (rc = tgmx_colsum(dy, ldx, R, D, d->ln1_b, 0, cs_ws, stream))) return rc;
  if (!attn) return TGMX_OK;
  if ((rc = tgmx_add_cols(g, ldx, du, ldx, R, D, 1, stream))) return rc;  // g <- dx1 = the LayerNorm's backward + the residual
  // the attention block
  const float* g1 = g;
  if (dropping) {
    if ((rc = tgmx_dropout(g, ldx, R, D, &site[1], gt, ldx, stream))) return rc;
    g1 = gt;
  }
  if (d->out_w && (rc = tgmx_sgemm_tn(g1, ldx, att, ldx, d->out_w, D, R, D, D, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
  if (d->out_b && (rc = tgmx_colsum(g1, ldx, R, D, d->out_b, 0, cs_ws, stream))) return rc;
  if (!(d->ln0_g || d->ln0_b || d->in_w || d->in_b || dx)) return TGMX_OK;
  if ((rc = tgmx_sgemm_nt_ep(g1, ldx, tr->out_wT, D, datt, ldx, R, D, D, nullptr, 0, nullptr, 0, stream))) return rc;
  if ((rc = tgmx_mha_small_backward(qkv, ldq, datt, ldx, B, T, H, D / H, dqkv, &site[0], stream))) return rc;
  if (d->in_w) {
    if ((rc = tgmx_layernorm_rows(x, ldx, R, D, ly->ln0_g, ly->ln0_b, eps, y, ldx, stream))) return rc;
    if ((rc = tgmx_sgemm_tn(dqkv, ldq, y, ldx, d->in_w, D, R, 3 * D, D, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
  }
  if (d->in_b && (rc = tgmx_colsum(dqkv, ldq, R, 3 * D, d->in_b, 0, cs_ws, stream))) return rc;
  if (!(d->ln0_g || d->ln0_b || dx)) return TGMX_OK;
  if ((rc = tgmx_sgemm_nt_ep(dqkv, ldq, tr->in_wT, 3 * D, dy, ldx, R, D, 3 * D, nullptr, 0, nullptr, 0, stream))) return rc;
  if ((rc = tgmx_ln_backward(dy, ldx, x, ldx, zero, 0, ly->ln0_g, D, eps, R, du, ldx, dgx, ldx, stream))) return rc;
  if (d->ln0_g && (rc = tgmx_colsum(dgx, ldx, R, D, d->ln0_g, 0, cs_ws, stream))) return rc;
  if (d->ln0_b && (rc = tgmx_colsum(dy, ldx, R, D, d->ln0_b, 0, cs_ws, stream))) return rc;
  if (!dx) return TGMX_OK;
  if ((rc = tgmx_add_cols(dx, ldx, du, ldx, R, D, 0, stream))) return rc;
  return tgmx_add_cols(dx, ldx, g, ldx, R, D, 1, stream);
}

static int layer_check(const tgmx_dygformer_layer_t* ly, const tgmx_dygformer_layer_tr_t* tr, const tgmx_dygformer_layer_grad_t* d, int64_t B, int T,
                       int H, int D, int64_t ldx, int64_t ldq, int64_t ldh, const tgmx_dropout_t* drop) {
  TGMX_REQUIRE(ly && tr && d && B >= 0 && T > 0 && H > 0 && D > 0 && D % H == 0 && ldx >= D && ldq >= 3ll * D && ldh >= 4ll * D && ldx % 4 == 0 &&
                   ldq % 4 == 0 && ldh % 4 == 0 && drop_ok(drop),
               "dygformer_layer_backward: bad sizes B=%lld T=%d H=%d D=%d (leading dimensions: multiples of 4)", (long long)B, T, H, D);
  return TGMX_OK;
}

extern "C" size_t tgmx_dygformer_layer_backward_workspace_bytes(int64_t B, int32_t T, int32_t D, int64_t ldx, int64_t ldq, int64_t ldh) {
  if (B < 0 || T <= 0 || D <= 0 || ldx < D || ldq < 3ll * D || ldh < 4ll * D) return 0;
  size_t need = 0;
  const tgmx_dropout_t on{0.5f, 0, 0, 0};  // (the size with dropout: an upper bound)
  layer_backward_pass(nullptr, nullptr, nullptr, B, T, 1, D, 0.f, nullptr, nullptr, nullptr, nullptr, ldx, ldq, ldh, nullptr, nullptr, &on, nullptr, true,
                      &need, nullptr);
  return need;
}

extern "C" int tgmx_dygformer_layer_backward(const tgmx_dygformer_layer_t* ly, const tgmx_dygformer_layer_tr_t* tr,
                                             const tgmx_dygformer_layer_grad_t* d, int64_t B, int32_t T, int32_t H, int32_t D, float eps,
                                             const float* x, const float* qkv, const float* att, const float* x1, int64_t ldx, int64_t ldq,
                                             int64_t ldh, float* g, float* dx, const tgmx_dropout_t* drop, void* workspace,
                                             size_t workspace_bytes, tgmx_stream_t stream) {
  int rc;
  if ((rc = layer_check(ly, tr, d, B, T, H, D, ldx, ldq, ldh, drop))) return rc;
  if (!tgmx_mha_small_train_supported(T, D / H)) {
    set_error("dygformer_layer_backward: T=%d tokens x head dimension %d is outside the attention backward's envelope", T, D / H);
    return TGMX_E_UNSUPPORTED;
  }
  if (B == 0) return TGMX_OK;
  TGMX_REQUIRE(x && qkv && att && x1 && g && g != dx, "dygformer_layer_backward: null or aliased pointer");
  TGMX_REQUIRE(ly->ln0_g && ly->ln0_b && ly->ln1_g && ly->ln1_b && ly->w1 && ly->b1 && tr->in_wT && tr->out_wT && tr->w1T && tr->w2T,
               "dygformer_layer_backward: the layer's weights or their transposes are missing");
  const size_t need = tgmx_dygformer_layer_backward_workspace_bytes(B, T, D, ldx, ldq, ldh);
  TGMX_REQUIRE(workspace && workspace_bytes >= need, "dygformer_layer_backward: workspace too small (%zu bytes, %zu needed)", workspace_bytes, need);
  size_t used = 0;
  return layer_backward_pass(ly, tr, d, B, T, H, D, eps, x, qkv, att, x1, ldx, ldq, ldh, g, dx, drop, workspace, false, &used, stream);
}

// ---- the whole backward as one call ---------------------------------------------------------------------------------------------------------
static bool layer_wanted(const tgmx_dygformer_layer_grad_t& d) {
  return d.ln0_g || d.ln0_b || d.in_w || d.in_b || d.out_w || d.out_b || d.ln1_g || d.ln1_b || d.w1 || d.b1 || d.w2 || d.b2;
}

static int dyg_bwd_check(const tgmx_dygformer_bwd_t* a, const char* what) {
  TGMX_REQUIRE(a, "%s: null argument block", what);
  TGMX_REQUIRE(a->P >= 0 && a->P < (1ll << 30) && a->S >= 0 && a->k >= 0 && a->k < 2048 && a->patch > 0 && (a->k + 1) % a->patch == 0 && a->C > 0 &&
                   a->heads > 0 && (4 * a->C) % a->heads == 0 && a->dN > 0 && a->dE > 0 && a->dT > 0 && a->E > 0 && a->num_layers >= 0 &&
                   a->num_layers <= TGMX_DYGFORMER_MAX_LAYERS,
               "%s: bad sizes", what);
  TGMX_REQUIRE(a->P == 0 || (a->ldg >= a->E && a->ldx >= 4 * a->C && a->ldx % 4 == 0 && a->ldq >= 12 * a->C && a->ldq % 4 == 0 && a->ldh >= 16 * a->C &&
                             a->ldh % 4 == 0 && a->ldch[0] >= a->dN && a->ldch[1] >= a->dE && a->ldch[2] >= a->dT && a->ldch[3] >= a->C),
               "%s: leading dimensions", what);
  TGMX_REQUIRE(a->drop_p >= 0.f && a->drop_p < 1.f, "%s: p must be in [0, 1)", what);
  return TGMX_OK;
}

static int dyg_backward_pass(const tgmx_dygformer_bwd_t* a, bool dry, size_t* need, tgmx_stream_t stream) {
  const int64_t P = a->P;
  const int L = a->k + 1, Np = L / a->patch, C = a->C, D = 4 * C, E = a->E, nL = a->num_layers, T = 2 * Np;
  const int64_t R = 2 * P * Np, n = 2 * P * L, ldx = a->ldx;
  const int dims[4] = {a->dN, a->dE, a->dT, C};
  const bool want_time = a->d_tw || a->d_tb, want_co = a->d_co_w1 || a->d_co_b1 || a->d_co_w2 || a->d_co_b2;
  bool want_proj = want_time || want_co;
  for (int c = 0; c < 4; ++c) want_proj = want_proj || a->d_proj_w[c] || a->d_proj_b[c];
  int lowest = nL;
  if (want_proj) lowest = 0;
  else
    for (int l = 0; l < nL; ++l)
      if (layer_wanted(a->d_layers[l])) {
        lowest = l;
        break;
      }
  const bool chain = want_proj || lowest < nL;

  WorkspaceCarver ws(dry ? nullptr : a->workspace);
  float* dmean = ws.take<float>(chain ? (size_t)2 * P * ldx : 0);
  float* gz = ws.take<float>(chain ? (size_t)R * ldx : 0);
  float* gz2 = ws.take<float>(chain && nL > lowest ? (size_t)R * ldx : 0);
  const int64_t ldt = a->ldch[2], ldf = a->ldch[3];
  float* dtime = ws.take<float>(want_time ? (size_t)n * ldt : 0);
  float* trows = ws.take<float>(want_time ? (size_t)n * 2 * a->dT : 0);
  float* dfeat = ws.take<float>(want_co ? (size_t)n * ldf : 0);
  const size_t co_bytes = want_co ? tgmx_dygformer_cooccurrence_backward_workspace_bytes(n, L, C) : 0;
  char* co_ws = ws.take<char>(co_bytes);
  const size_t ly_bytes = nL > lowest ? tgmx_dygformer_layer_backward_workspace_bytes(P, T, D, ldx, a->ldq, a->ldh) : 0;
  char* ly_ws = ws.take<char>(ly_bytes);
  size_t tn = tgmx_sgemm_tn_workspace_bytes(2 * P, E, D, 1);
  for (int c = 0; c < 4; ++c) {
    const size_t b = tgmx_sgemm_tn_workspace_bytes(R, C, dims[c], 1);
    tn = b > tn ? b : tn;
  }
  float* tn_ws = ws.take<float>(tn / sizeof(float) + 1);
  int widest = E > D ? E : D;
  widest = 2 * a->dT > widest ? 2 * a->dT : widest;
  float* cs_ws = ws.take<float>((size_t)256 * widest);
  *need = ws.total();
  if (dry) return TGMX_OK;

  int rc;
  // 1. the output layer
  if (a->d_out_w && (rc = tgmx_sgemm_tn(a->g, a->ldg, a->mean, ldx, a->d_out_w, D, 2 * P, E, D, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
  if (a->d_out_b && (rc = tgmx_colsum(a->g, a->ldg, 2 * P, E, a->d_out_b, 0, cs_ws, stream))) return rc;
  if (!chain) return TGMX_OK;
  // 2. the patch mean
  if ((rc = tgmx_sgemm_nt_ep(a->g, a->ldg, a->out_wT, E, dmean, ldx, 2 * P, D, E, nullptr, 0, nullptr, 0, stream))) return rc;
  if ((rc = tgmx_dygformer_mean_backward(dmean, ldx, P, Np, D, gz, ldx, stream))) return rc;
  // 3. the layers, last first
  for (int l = nL - 1; l >= lowest; --l) {
    const int64_t ox = (int64_t)l * R * ldx, oq = (int64_t)l * R * a->ldq;
    const bool down = l > lowest || want_proj;
    const tgmx_dropout_t d{a->drop_p, a->drop_seed, a->drop_stream + 4ull * l, 0};
    if ((rc = tgmx_dygformer_layer_backward(&a->layers[l], &a->tr[l], &a->d_layers[l], P, T, a->heads, D, a->eps, a->save_x + ox, a->save_qkv + oq,
                                            a->save_att + ox, a->save_x1 + ox, ldx, a->ldq, a->ldh, gz, down ? gz2 : nullptr, &d, ly_ws, ly_bytes,
                                            stream)))
      return rc;
    float* tmp = gz;
    gz = gz2;
    gz2 = tmp;
  }
  if (!want_proj) return TGMX_OK;
  // 4. the four projections: channel c's tokens are [R, patch ldch[c]]; slot s of a patch is the column range [s ldch, s ldch + d)
  for (int c = 0; c < 4; ++c) {
    const int64_t ld = a->ldch[c], Kc = (int64_t)a->patch * ld;
    if (a->d_proj_w[c])
      for (int s = 0; s < a->patch; ++s)
        if ((rc = tgmx_sgemm_tn(gz + (int64_t)c * C, ldx, a->ch[c] + s * ld, Kc, a->d_proj_w[c] + (int64_t)s * dims[c], (int64_t)a->patch * dims[c], R, C,
                                dims[c], 1, 0, 0, 0, 0, tn_ws, stream)))
          return rc;
    if (a->d_proj_b[c] && (rc = tgmx_colsum(gz + (int64_t)c * C, ldx, R, C, a->d_proj_b[c], 0, cs_ws, stream))) return rc;
  }
  // 5. the time and co-occurrence tails
  if (want_time) {
    const int64_t Kc = (int64_t)a->patch * ldt;
    if ((rc = tgmx_sgemm_nt_ep(gz + 2ll * C, ldx, a->proj_wT[2], C, dtime, Kc, R, (int)Kc, C, nullptr, 0, nullptr, 0, stream))) return rc;
    if ((rc = tgmx_dygformer_time_backward(dtime, ldt, a->src, a->dst, a->edge_time, P, a->nbr_nids, a->nbr_t, a->S, a->k, a->src_rows, a->dst_rows, a->tw,
                                           a->tb, a->dT, trows, stream)))
      return rc;
    if (a->d_tw && (rc = tgmx_colsum(trows, 2 * a->dT, n, a->dT, a->d_tw, 0, cs_ws, stream))) return rc;
    if (a->d_tb && (rc = tgmx_colsum(trows + a->dT, 2 * a->dT, n, a->dT, a->d_tb, 0, cs_ws, stream))) return rc;
  }
  if (want_co) {
    const int64_t Kc = (int64_t)a->patch * ldf;
    if ((rc = tgmx_sgemm_nt_ep(gz + 3ll * C, ldx, a->proj_wT[3], C, dfeat, Kc, R, (int)Kc, C, nullptr, 0, nullptr, 0, stream))) return rc;
    if ((rc = tgmx_dygformer_cooccurrence_backward(a->counts, dfeat, ldf, n, L, C, a->co_w1, a->co_b1, a->co_w2T, a->d_co_w1, a->d_co_b1, a->d_co_w2,
                                                   a->d_co_b2, co_ws, co_bytes, stream)))
      return rc;
  }
  return TGMX_OK;
}

extern "C" size_t tgmx_dygformer_backward_workspace_bytes(const tgmx_dygformer_bwd_t* a) {
  size_t need = 0;
  if (dyg_bwd_check(a, "dygformer_backward_workspace_bytes") != TGMX_OK) return 0;
  return dyg_backward_pass(a, true, &need, nullptr) == TGMX_OK ? need : 0;
}

extern "C" int tgmx_dygformer_backward(const tgmx_dygformer_bwd_t* a, tgmx_stream_t stream) {
  int rc;
  if ((rc = dyg_bwd_check(a, "dygformer_backward"))) return rc;
  if (a->P == 0) return TGMX_OK;
  if (!tgmx_mha_small_train_supported(2 * ((a->k + 1) / a->patch), 4 * a->C / a->heads)) {
    set_error("dygformer_backward: %d tokens x head dimension %d is outside the attention backward's envelope", 2 * ((a->k + 1) / a->patch),
              4 * a->C / a->heads);
    return TGMX_E_UNSUPPORTED;
  }
  TGMX_REQUIRE(a->g && a->mean && a->out_wT, "dygformer_backward: the upstream gradient or the forward's saved buffers are missing");
  TGMX_REQUIRE(a->num_layers == 0 || (a->save_x && a->save_qkv && a->save_att && a->save_x1), "dygformer_backward: the layers' saved buffers are missing");
  for (int c = 0; c < 4; ++c) TGMX_REQUIRE(!a->d_proj_w[c] || a->ch[c], "dygformer_backward: d_proj_w[%d] needs ch[%d]", c, c);
  TGMX_REQUIRE(!(a->d_tw || a->d_tb) || (a->proj_wT[2] && a->tw && a->tb && a->src && a->dst && a->edge_time),
               "dygformer_backward: the time tail needs proj_wT[2], the time encoder and the call's ids and times");
  TGMX_REQUIRE(!(a->d_co_w1 || a->d_co_b1 || a->d_co_w2 || a->d_co_b2) || (a->proj_wT[3] && a->counts && a->co_w1 && a->co_b1 && a->co_w2T),
               "dygformer_backward: the co-occurrence tail needs proj_wT[3], the counts and the encoder");
  size_t need = 0;
  if ((rc = dyg_backward_pass(a, true, &need, nullptr))) return rc;
  TGMX_REQUIRE(a->workspace && a->workspace_bytes >= need, "dygformer_backward: workspace too small (%zu bytes, %zu needed)", a->workspace_bytes, need);
  return dyg_backward_pass(a, false, &need, stream);
}
