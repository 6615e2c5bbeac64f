// GraphMixer / MLPMixer training: the backward of tgmx_graphmixer_forward_train (csrc/mixer.hip) as one call, and its pieces.
//
//   tgmx_mixer_token_backward   the token block: one workgroup per seed, one thread per channel; recomputes the column's LayerNorm over K,
//                               the hidden pre-activations and GELU; writes dx and, per column, the rows the parameter gradients are sums of
//   tgmx_mixer_gelu_backward    the channel FFN's GELU' (exact erf) with the site's dropout mask, in place
//   tgmx_mixer_tail_backward    the link mean over the valid slots
//   tgmx_mixer_channel_norm     y = LN_C(z1) again, from the saved z1
//   tgmx_graphmixer_backward    the whole chain; GEMMs and reductions are the dense library's (tgmx_sgemm_nt_ep, tgmx_sgemm_tn, tgmx_colsum,
//                               tgmx_ln_backward, tgmx_add_cols, tgmx_dropout)
//
// No float atomics anywhere: every sum over seeds and channels goes through tgmx_sgemm_tn / tgmx_colsum, whose orders are fixed.
#include <math.h>

#include "common.h"
#include "edge_csr.h"

namespace tgmx {

__device__ __forceinline__ float gelu_erf_fwd(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }
// d/dv [v Phi(v)] = Phi(v) + v phi(v)
__device__ __forceinline__ float gelu_erf_grad(float v) {
  return 0.5f * (1.f + erff(v * 0.70710678118654752f)) + v * 0.3989422804014327f * expf(-0.5f * v * v);
}

// ---- token block ------------------------------------------------------------------------------------------------------------------------------
// Per thread (one channel c of seed s; chunks of kThreads channels) the column's values live in LDS at [feature][thread], pitch
// kThreads + 1 floats: in the compute phase a wave reads consecutive floats of one feature, in the write-out phase consecutive features
// of one thread, kThreads + 1 floats apart -- neither meets a bank twice (64 banks of 4 bytes).  The features are laid out in the order
// of a row of `rows`, so the write-out is a transposed copy: the chunk's n rows are one contiguous range of n ldw floats.
// kThreads: 128, or 64 / 32 where 4 K + 2 Ht values a column at the wider pitch would not fit 64 KiB (K = 20 at Ht = 26 takes 64).
template <int kThreads>
__global__ __launch_bounds__(kThreads) void mixer_token_backward_kernel(
    const float* __restrict__ x, long long ldx, const float* __restrict__ dz1, long long ldd, int K, int C, const float* __restrict__ tg,
    const float* __restrict__ tbeta, const float* __restrict__ w1, const float* __restrict__ b1, int Ht, const float* __restrict__ w2, float eps,
    float* __restrict__ dx, long long ldo, float* __restrict__ rows, long long ldw, const DropoutArgs d0, const DropoutArgs d1) {
  extern __shared__ float lds[];
  constexpr int P = kThreads + 1;
  float* __restrict__ DO = lds;                  // [K]: the output gradient, dropped
  float* __restrict__ XN = DO + (size_t)K * P;   // [K]: the LayerNorm's output
  float* __restrict__ DXN = XN + (size_t)K * P;  // [K]: its gradient
  float* __restrict__ XH = DXN + (size_t)K * P;  // [K]: x, then x-hat, then dxn x-hat
  float* __restrict__ HD = XH + (size_t)K * P;   // [Ht]: the hidden activations, dropped
  float* __restrict__ DA = HD + (size_t)Ht * P;  // [Ht]: the pre-activations, then their gradient
  const int W = 4 * K + 2 * Ht;
  const long long s = blockIdx.x;
  const int t = threadIdx.x;
  const float* __restrict__ xs = x + s * K * ldx;
  const float* __restrict__ ds = dz1 + s * K * ldd;
  float* __restrict__ os = dx + s * K * ldo;
  const float invK = 1.f / (float)K;
  for (int c0 = 0; c0 < C; c0 += kThreads) {
    const int c = c0 + t;
    if (c < C) {
      const unsigned long long col = (unsigned long long)s * C + c;
      // both columns are read once, all 2 K loads in flight together
#pragma unroll 8
      for (int k = 0; k < K; ++k) XH[k * P + t] = xs[k * ldx + c];
#pragma unroll 8
      for (int k = 0; k < K; ++k) DO[k * P + t] = ds[k * ldd + c];
      // the forward's LayerNorm over the K tokens (the plain mean, as GraphMixer's forward takes it)
      float sum = 0.f;
      for (int k = 0; k < K; ++k) sum += XH[k * P + t];
      const float mean = sum / (float)K;
      float var = 0.f;
      for (int k = 0; k < K; ++k) {
        const float d = XH[k * P + t] - mean;
        var = __fmaf_rn(d, d, var);
      }
      const float rstd = 1.f / sqrtf(var / (float)K + eps);
      for (int k = 0; k < K; ++k) {
        const float xh = (XH[k * P + t] - mean) * rstd;
        XH[k * P + t] = xh;
        XN[k * P + t] = xh * tg[k] + tbeta[k];
        DO[k * P + t] *= dropout_scale(d1, col * K + k);
      }
      for (int j = 0; j < Ht; ++j) {
        float a = 0.f;
        for (int k = 0; k < K; ++k) a = __fmaf_rn(w1[j * K + k], XN[k * P + t], a);
        a += b1[j];
        const float m = dropout_scale(d0, col * Ht + j);
        float dh = 0.f;
        for (int k = 0; k < K; ++k) dh = __fmaf_rn(w2[k * Ht + j], DO[k * P + t], dh);
        HD[j * P + t] = gelu_erf_fwd(a) * m;
        DA[j * P + t] = dh * m * gelu_erf_grad(a);
      }
      // dxn = W1^T da; the LayerNorm's backward over K: dx = rstd (g dxn - mean(g dxn) - xhat mean(g dxn xhat)) + the residual
      float m1 = 0.f, m2 = 0.f;
      for (int k = 0; k < K; ++k) {
        float a = 0.f;
        for (int j = 0; j < Ht; ++j) a = __fmaf_rn(w1[j * K + k], DA[j * P + t], a);
        DXN[k * P + t] = a;
        const float gk = a * tg[k];
        m1 += gk;
        m2 = __fmaf_rn(gk, XH[k * P + t], m2);
      }
      m1 *= invK;
      m2 *= invK;
      for (int k = 0; k < K; ++k) {
        const float xh = XH[k * P + t], dxn = DXN[k * P + t];
        // (the residual takes the gradient as it came, before the output's dropout: read again, a cache hit)
        os[k * ldo + c] = rstd * (dxn * tg[k] - m1 - xh * m2) + ds[k * ldd + c];
        XH[k * P + t] = dxn * xh;
      }
    }
    if (rows) {  // (uniform over the workgroup)
      __syncthreads();
      const int n = C - c0 < kThreads ? C - c0 : kThreads;
      float* __restrict__ dst = rows + ((long long)s * C + c0) * ldw;
      const int total = n * (int)ldw;
      for (int i = t; i < total; i += kThreads) {
        const int r = i / (int)ldw, f = i - r * (int)ldw;
        dst[i] = f < W ? lds[f * P + r] : 0.f;
      }
      __syncthreads();
    }
  }
}

// ---- the small pieces ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mixer_gelu_backward_kernel(float* __restrict__ a, long long lda, float* __restrict__ dh, long long ldh,
                                                                  long long R, int C, const DropoutArgs d) {
  const long long total = R * C;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
    const long long r = e / C;
    const int c = (int)(e - r * C);
    const float v = a[r * lda + c], m = dropout_scale(d, (unsigned long long)e);
    a[r * lda + c] = gelu_erf_fwd(v) * m;
    dh[r * ldh + c] = dh[r * ldh + c] * m * gelu_erf_grad(v);
  }
}

// one workgroup per seed
__global__ __launch_bounds__(256) void mixer_tail_backward_kernel(const float* __restrict__ dcat, long long ldc, const int32_t* __restrict__ nbr_nids,
                                                                  int K, int C, float* __restrict__ dz, long long ldz) {
  const long long s = blockIdx.x;
  int valid = 0;
  for (int k = 0; k < K; ++k) valid += nbr_nids[s * K + k] != -1;
  const float denom = (float)(valid > 0 ? valid : 1);
  const float* __restrict__ g = dcat + s * ldc;
  const int total = K * C;
  for (int e = threadIdx.x; e < total; e += blockDim.x) {
    const int k = e / C, c = e - k * C;
    dz[(s * K + k) * ldz + c] = nbr_nids[s * K + k] != -1 ? g[c] / denom : 0.f;
  }
}

// one wave per row: pass 2 of mixer_token_kernel, reading the row from global memory
__global__ __launch_bounds__(256) void mixer_channel_norm_kernel(const float* __restrict__ z1, long long ldz, long long R, int C,
                                                                 const float* __restrict__ cg, const float* __restrict__ cb, float eps,
                                                                 float* __restrict__ y, long long ldy) {
  const int lane = lane_id();
  const long long r = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (r >= R) return;
  const float* __restrict__ row = z1 + r * ldz;
  float sum = 0.f;
  for (int c = lane; c < C; c += kWave) sum += row[c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  const float mean = sum / (float)C;
  float var = 0.f;
  for (int c = lane; c < C; c += kWave) {
    const float d = row[c] - mean;
    var = __fmaf_rn(d, d, var);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) var += __shfl_xor(var, o);
  const float rstd = 1.f / sqrtf(var / (float)C + eps);
  float* __restrict__ yo = y + r * ldy;
  for (int c = lane; c < C; c += kWave) yo[c] = (row[c] - mean) * rstd * cg[c] + cb[c];
}

static unsigned mixer_blocks(long long total) {
  long long blocks = (total + 255) / 256;
  return (unsigned)(blocks > 16384 ? 16384 : (blocks < 1 ? 1 : blocks));
}

static bool drop_ok(const tgmx_dropout_t* d) { return !d || (d->p >= 0.f && d->p < 1.f); }

}  // namespace tgmx

using namespace tgmx;

extern "C" int tgmx_mixer_train_supported(int32_t K, int32_t C, int32_t Ht) {
  if (K <= 0 || C <= 0 || Ht < 0) return 0;
  return mixer_token_lds_bytes(K, C, Ht) <= kMixerTokMaxLds && mixer_token_bwd_threads(K, Ht) > 0 ? 1 : 0;
}

extern "C" int tgmx_mixer_token_backward(const float* x, int64_t ldx, const float* dz1, int64_t ldd, int64_t S, int32_t K, int32_t C,
                                         const float* tok_g, const float* tok_b, const float* w1, const float* b1, int32_t Ht, const float* w2,
                                         float eps, float* dx, int64_t ldo, float* rows, int64_t ldw, const tgmx_dropout_t* drop_hidden,
                                         const tgmx_dropout_t* drop_out, tgmx_stream_t stream) {
  TGMX_REQUIRE(S >= 0 && S < (1ll << 31) && K > 0 && C > 0 && Ht >= 0 && ldx >= C && ldd >= C && ldo >= C,
               "mixer_token_backward: bad sizes S=%lld K=%d C=%d Ht=%d", (long long)S, K, C, Ht);
  TGMX_REQUIRE(!rows || (ldw >= 4 * K + 2 * Ht && ldw < (1 << 20)), "mixer_token_backward: rows of %lld floats, %d needed", (long long)ldw, 4 * K + 2 * Ht);
  TGMX_REQUIRE(drop_ok(drop_hidden) && drop_ok(drop_out), "mixer_token_backward: p must be in [0, 1)");
  if (S == 0) return TGMX_OK;
  TGMX_REQUIRE(x && dz1 && dx && dx != dz1 && tok_g && tok_b && (Ht == 0 || (w1 && b1 && w2)), "mixer_token_backward: null or aliased pointer");
  const int threads = mixer_token_bwd_threads(K, Ht);
  if (threads == 0) {
    set_error("mixer_token_backward: K=%d tokens (token hidden %d) need %zu bytes of LDS per workgroup at 32 channels a pass, more than %zu", K, Ht,
              mixer_token_bwd_lds_bytes(K, Ht, 32), kMixerTokMaxLds);
    return TGMX_E_UNSUPPORTED;
  }
  const size_t lds = mixer_token_bwd_lds_bytes(K, Ht, threads);
  const DropoutArgs d0 = make_dropout(drop_hidden), d1 = make_dropout(drop_out);
#define TGMX_TOKEN_BWD(T)                                                                                                                        \
  hipLaunchKernelGGL(mixer_token_backward_kernel<T>, dim3((unsigned)S), dim3(T), lds, (hipStream_t)stream, x, (long long)ldx, dz1, (long long)ldd, \
                     K, C, tok_g, tok_b, w1, b1, Ht, w2, eps, dx, (long long)ldo, rows, (long long)ldw, d0, d1)
  if (threads == 128) TGMX_TOKEN_BWD(128);
  else if (threads == 64) TGMX_TOKEN_BWD(64);
  else TGMX_TOKEN_BWD(32);
#undef TGMX_TOKEN_BWD
  TGMX_CHECK_LAUNCH("mixer_token_backward");
  return TGMX_OK;
}

extern "C" int tgmx_mixer_gelu_backward(float* a, int64_t lda, float* dh, int64_t ldh, int64_t R, int32_t C, const tgmx_dropout_t* drop,
                                        tgmx_stream_t stream) {
  TGMX_REQUIRE(R >= 0 && C > 0 && lda >= C && ldh >= C && drop_ok(drop), "mixer_gelu_backward: bad sizes R=%lld C=%d", (long long)R, C);
  if (R == 0) return TGMX_OK;
  TGMX_REQUIRE(a && dh && a != dh, "mixer_gelu_backward: null or aliased pointer");
  hipLaunchKernelGGL(mixer_gelu_backward_kernel, dim3(mixer_blocks((long long)R * C)), dim3(256), 0, (hipStream_t)stream, a, (long long)lda, dh,
                     (long long)ldh, (long long)R, C, make_dropout(drop));
  TGMX_CHECK_LAUNCH("mixer_gelu_backward");
  return TGMX_OK;
}

extern "C" int tgmx_mixer_tail_backward(const float* dcat, int64_t ldc, const int32_t* nbr_nids, int64_t S, int32_t K, int32_t C, float* dz,
                                        int64_t ldz, tgmx_stream_t stream) {
  TGMX_REQUIRE(S >= 0 && S < (1ll << 31) && K > 0 && C > 0 && (long long)K * C < (1ll << 31) && ldc >= C && ldz >= C,
               "mixer_tail_backward: bad sizes S=%lld K=%d C=%d", (long long)S, K, C);
  if (S == 0) return TGMX_OK;
  TGMX_REQUIRE(dcat && nbr_nids && dz, "mixer_tail_backward: null pointer");
  hipLaunchKernelGGL(mixer_tail_backward_kernel, dim3((unsigned)S), dim3(256), 0, (hipStream_t)stream, dcat, (long long)ldc, nbr_nids, K, C, dz,
                     (long long)ldz);
  TGMX_CHECK_LAUNCH("mixer_tail_backward");
  return TGMX_OK;
}

extern "C" int tgmx_mixer_channel_norm(const float* z1, int64_t ldz, int64_t R, int32_t C, const float* gamma, const float* beta, float eps,
                                       float* y, int64_t ldy, tgmx_stream_t stream) {
  TGMX_REQUIRE(R >= 0 && R < (1ll << 32) && C > 0 && ldz >= C && ldy >= C, "mixer_channel_norm: bad sizes R=%lld C=%d", (long long)R, C);
  if (R == 0) return TGMX_OK;
  TGMX_REQUIRE(z1 && gamma && beta && y, "mixer_channel_norm: null pointer");
  hipLaunchKernelGGL(mixer_channel_norm_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, z1, (long long)ldz, (long long)R, C,
                     gamma, beta, eps, y, (long long)ldy);
  TGMX_CHECK_LAUNCH("mixer_channel_norm");
  return TGMX_OK;
}

// ---- the channel block of a layer (shared with csrc/tpnet_bwd.hip) -------------------------------------------------------------------------------
int tgmx::mixer_channel_backward(const tgmx_mixer_layer_t& ly, const tgmx_mixer_layer_grad_t& d, const float* ch_w1T, const float* ch_w2T,
                                 const float* z1, const float* gz, int64_t R, int32_t D, int64_t ldz, int64_t ldh, float eps,
                                 const tgmx_dropout_t* site, bool down, const MixerChannelBufs& b, tgmx_stream_t stream) {
  const int hc = ly.ch_hidden;
  const bool dropping = site[3].p > 0.f;
  float *abuf = b.abuf, *hbuf = b.hbuf, *y = b.y, *dy = b.dy, *du = b.du, *dgx = b.dgx, *gt = b.gt, *tn_ws = b.tn_ws, *cs_ws = b.cs_ws;
  int rc;
  if ((rc = tgmx_mixer_channel_norm(z1, ldz, R, D, ly.ch_g, ly.ch_b, eps, y, ldz, stream))) return rc;
  if ((rc = tgmx_sgemm_nt_ep(y, ldz, ly.ch_w1, D, abuf, ldh, R, hc, D, ly.ch_b1, 0, nullptr, 0, stream))) return rc;
  const float* g3 = gz;
  if (dropping) {
    if ((rc = tgmx_dropout(gz, ldz, R, D, &site[3], gt, ldz, stream))) return rc;
    g3 = gt;
  }
  if ((rc = tgmx_sgemm_nt_ep(g3, ldz, ch_w2T, D, hbuf, ldh, R, hc, D, nullptr, 0, nullptr, 0, stream))) return rc;
  if ((rc = tgmx_mixer_gelu_backward(abuf, ldh, hbuf, ldh, R, hc, &site[2], stream))) return rc;
  if (d.ch_w2 && (rc = tgmx_sgemm_tn(g3, ldz, abuf, ldh, d.ch_w2, hc, R, D, hc, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
  if (d.ch_b2 && (rc = tgmx_colsum(g3, ldz, R, D, d.ch_b2, 0, cs_ws, stream))) return rc;
  if (d.ch_w1 && (rc = tgmx_sgemm_tn(hbuf, ldh, y, ldz, d.ch_w1, D, R, hc, D, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
  if (d.ch_b1 && (rc = tgmx_colsum(hbuf, ldh, R, hc, d.ch_b1, 0, cs_ws, stream))) return rc;
  if (d.ch_g || d.ch_b || down) {
    if ((rc = tgmx_sgemm_nt_ep(hbuf, ldh, ch_w1T, hc, dy, ldz, R, D, hc, nullptr, 0, nullptr, 0, stream))) return rc;
    if ((rc = tgmx_ln_backward(dy, ldz, z1, ldz, b.zero, 0, ly.ch_g, D, eps, R, du, ldz, dgx, ldz, stream))) return rc;
    if (d.ch_g && (rc = tgmx_colsum(dgx, ldz, R, D, d.ch_g, 0, cs_ws, stream))) return rc;
    if (d.ch_b && (rc = tgmx_colsum(dy, ldz, R, D, d.ch_b, 0, cs_ws, stream))) return rc;
  }
  if (!down) return TGMX_OK;
  return tgmx_add_cols(du, ldz, gz, ldz, R, D, 1, stream);  // dz1 = the LayerNorm's backward + the residual
}

// ---- the whole backward as one call ---------------------------------------------------------------------------------------------------------
static bool tok_wanted(const tgmx_mixer_layer_grad_t& d) { return d.tok_g || d.tok_b || d.tok_w1 || d.tok_b1 || d.tok_w2 || d.tok_b2; }
static bool ch_wanted(const tgmx_mixer_layer_grad_t& d) { return d.ch_g || d.ch_b || d.ch_w1 || d.ch_b1 || d.ch_w2 || d.ch_b2; }

static int gm_bwd_check(const tgmx_graphmixer_bwd_t* a, const char* what) {
  TGMX_REQUIRE(a, "%s: null argument block", what);
  TGMX_REQUIRE(a->S >= 0 && a->S < (1ll << 31) && a->K > 0 && a->D > 0 && a->T > 0 && a->E > 0 && a->F > 0 && a->num_layers >= 0 &&
                   a->num_layers <= TGMX_MIXER_MAX_LAYERS && a->S * a->K * (long long)a->D < (1ll << 40),
               "%s: bad sizes", what);
  TGMX_REQUIRE(a->S == 0 || (a->ldg >= a->E && a->ldx0 >= a->D + a->T && a->ldz >= a->D && a->ldcat >= a->D + a->F), "%s: leading dimensions", what);
  TGMX_REQUIRE(a->drop_p >= 0.f && a->drop_p < 1.f, "%s: p must be in [0, 1)", what);
  for (int l = 0; l < a->num_layers; ++l)
    TGMX_REQUIRE(a->layers[l].ch_hidden > 0 && a->layers[l].tok_hidden >= 0 && (a->S == 0 || a->ldh >= a->layers[l].ch_hidden), "%s: layer %d's widths", what, l);
  return TGMX_OK;
}

// dry: lay the workspace out only (*need = its size), launch nothing
static int gm_backward_pass(const tgmx_graphmixer_bwd_t* a, bool dry, size_t* need, tgmx_stream_t stream) {
  const int64_t S = a->S, R = S * a->K, SC = S * a->D;
  const int K = a->K, D = a->D, T = a->T, E = a->E, F = a->F, L = a->num_layers;
  const int64_t ldz = a->ldz, ldh = a->ldh;
  const bool dropping = a->drop_p > 0.f;
  hipStream_t st = (hipStream_t)stream;
  // lowest: the lowest layer whose token block's input gradient, or a gradient of its own, somebody reads (L: only the output layer's)
  const bool want_proj = a->d_proj_w || a->d_proj_b;
  int lowest = L;
  bool below = want_proj;
  if (want_proj) lowest = 0;
  else
    for (int l = 0; l < L; ++l)
      if (tok_wanted(a->d_layers[l]) || ch_wanted(a->d_layers[l])) {
        lowest = l;
        below = true;
        break;
      }
  const bool chain = below;  // anything below the output layer
  int Hc = 1, Ht = 0;
  for (int l = 0; l < L; ++l) {
    Hc = a->layers[l].ch_hidden > Hc ? a->layers[l].ch_hidden : Hc;
    Ht = a->layers[l].tok_hidden > Ht ? a->layers[l].tok_hidden : Ht;
  }
  const int64_t ldw = (4 * K + 2 * Ht + 3) / 4 * 4;
  bool any_tok = false;
  for (int l = lowest; l < L; ++l) any_tok = any_tok || tok_wanted(a->d_layers[l]);

  WorkspaceCarver ws(dry ? nullptr : a->workspace);
  const size_t Rz = chain ? (size_t)R * ldz : 0, Rh = chain && L > lowest ? (size_t)R * ldh : 0, Rl = L > lowest ? Rz : 0;
  float* dcat = ws.take<float>(chain ? (size_t)S * ldz : 0);
  float* gz = ws.take<float>(Rz);
  float* gz2 = ws.take<float>(Rl);
  float* abuf = ws.take<float>(Rh);
  float* hbuf = ws.take<float>(Rh);
  float* y = ws.take<float>(Rl);
  float* dy = ws.take<float>(Rl);
  float* du = ws.take<float>(Rl);
  float* dgx = ws.take<float>(Rl);
  float* gt = ws.take<float>(dropping ? Rl : 0);
  float* zero = ws.take<float>((size_t)ldz);
  float* rows = ws.take<float>(any_tok ? (size_t)SC * ldw : 0);
  size_t tn_bytes = tgmx_sgemm_tn_workspace_bytes(S, E, D + F, 1);
  auto grow = [&](size_t b) { tn_bytes = b > tn_bytes ? b : tn_bytes; };
  grow(tgmx_sgemm_tn_workspace_bytes(R, D, D + T, 1));
  for (int l = lowest; l < L; ++l) {
    const tgmx_mixer_layer_t& ly = a->layers[l];
    grow(tgmx_sgemm_tn_workspace_bytes(R, D, ly.ch_hidden, 1));
    grow(tgmx_sgemm_tn_workspace_bytes(R, ly.ch_hidden, D, 1));
    if (ly.tok_hidden > 0) {
      grow(tgmx_sgemm_tn_workspace_bytes(SC, K, ly.tok_hidden, 1));
      grow(tgmx_sgemm_tn_workspace_bytes(SC, ly.tok_hidden, K, 1));
    }
  }
  float* tn_ws = ws.take<float>(tn_bytes / sizeof(float) + 1);
  int widest = E > D ? E : D;
  widest = Hc > widest ? Hc : widest;
  widest = K > widest ? K : widest;
  widest = Ht > widest ? Ht : widest;
  float* cs_ws = ws.take<float>((size_t)256 * widest);
  *need = ws.total();
  if (dry) return TGMX_OK;

  int rc;
  // 1. the output layer
  if (a->d_out_w && (rc = tgmx_sgemm_tn(a->g, a->ldg, a->cat, a->ldcat, a->d_out_w, D + F, S, E, D + F, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
  if (a->d_out_b && (rc = tgmx_colsum(a->g, a->ldg, S, E, a->d_out_b, 0, cs_ws, stream))) return rc;
  if (!chain) return TGMX_OK;
  // 2. the link mean
  if ((rc = tgmx_sgemm_nt_ep(a->g, a->ldg, a->out_wT, E, dcat, ldz, S, D, E, nullptr, 0, nullptr, 0, stream))) return rc;
  if ((rc = tgmx_mixer_tail_backward(dcat, ldz, a->nbr_nids, S, K, D, gz, ldz, stream))) return rc;
  // 3. the layers, last first
  if (L > lowest && hipMemsetAsync(zero, 0, (size_t)ldz * sizeof(float), st) != hipSuccess) {
    set_error("graphmixer_backward: hipMemsetAsync failed");
    return TGMX_E_LAUNCH;
  }
  const size_t per = (size_t)R * ldz;
  const MixerChannelBufs cb{abuf, hbuf, y, dy, du, dgx, gt, zero, tn_ws, cs_ws};
  for (int l = L - 1; l >= lowest; --l) {
    const tgmx_mixer_layer_t& ly = a->layers[l];
    const tgmx_mixer_layer_grad_t& d = a->d_layers[l];
    const int ht = ly.tok_hidden;
    const float* z_in = a->save_z + l * per;
    const float* z1 = a->save_z1 + l * per;
    const bool tok = tok_wanted(d), down = tok || l > lowest || want_proj;  // somebody reads dz1
    tgmx_dropout_t site[4];
    for (int s = 0; s < 4; ++s) site[s] = tgmx_dropout_t{a->drop_p, a->drop_seed, a->drop_stream + 4ull * l + s, 0};
    if ((rc = mixer_channel_backward(ly, d, a->ch_w1T[l], a->ch_w2T[l], z1, gz, R, D, ldz, ldh, a->eps, site, down, cb, stream))) return rc;
    if (!down) break;
    // the token block
    if ((rc = tgmx_mixer_token_backward(z_in, ldz, du, ldz, S, K, D, ly.tok_g, ly.tok_b, ly.tok_w1, ly.tok_b1, ht, ly.tok_w2, a->eps, gz2, ldz,
                                        tok ? rows : nullptr, ldw, &site[0], &site[1], stream)))
      return rc;
    if (tok) {
      const float *r_do = rows, *r_xn = rows + K, *r_dxn = rows + 2 * K, *r_gxh = rows + 3 * K, *r_hd = rows + 4 * K, *r_da = rows + 4 * K + ht;
      if (ht > 0) {
        if (d.tok_w2 && (rc = tgmx_sgemm_tn(r_do, ldw, r_hd, ldw, d.tok_w2, ht, SC, K, ht, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
        if (d.tok_w1 && (rc = tgmx_sgemm_tn(r_da, ldw, r_xn, ldw, d.tok_w1, K, SC, ht, K, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
        if (d.tok_b1 && (rc = tgmx_colsum(r_da, ldw, SC, ht, d.tok_b1, 0, cs_ws, stream))) return rc;
      }
      if (d.tok_b2 && (rc = tgmx_colsum(r_do, ldw, SC, K, d.tok_b2, 0, cs_ws, stream))) return rc;
      if (d.tok_b && (rc = tgmx_colsum(r_dxn, ldw, SC, K, d.tok_b, 0, cs_ws, stream))) return rc;
      if (d.tok_g && (rc = tgmx_colsum(r_gxh, ldw, SC, K, d.tok_g, 0, cs_ws, stream))) return rc;
    }
    float* tmp = gz;
    gz = gz2;
    gz2 = tmp;
  }
  // 4. the projection
  if (a->d_proj_w && (rc = tgmx_sgemm_tn(gz, ldz, a->x0, a->ldx0, a->d_proj_w, D + T, R, D, D + T, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
  if (a->d_proj_b && (rc = tgmx_colsum(gz, ldz, R, D, a->d_proj_b, 0, cs_ws, stream))) return rc;
  return TGMX_OK;
}

extern "C" size_t tgmx_graphmixer_backward_workspace_bytes(const tgmx_graphmixer_bwd_t* a) {
  size_t need = 0;
  if (gm_bwd_check(a, "graphmixer_backward_workspace_bytes") != TGMX_OK) return 0;
  return gm_backward_pass(a, true, &need, nullptr) == TGMX_OK ? need : 0;
}

extern "C" int tgmx_graphmixer_backward(const tgmx_graphmixer_bwd_t* a, tgmx_stream_t stream) {
  int rc;
  if ((rc = gm_bwd_check(a, "graphmixer_backward"))) return rc;
  if (a->S == 0) return TGMX_OK;
  TGMX_REQUIRE(a->g && a->cat && a->nbr_nids && a->out_wT, "graphmixer_backward: the upstream gradient or the forward's saved buffers are missing");
  TGMX_REQUIRE(a->num_layers == 0 || (a->save_z && a->save_z1), "graphmixer_backward: the layers' saved inputs are missing");
  TGMX_REQUIRE(!a->d_proj_w || a->x0, "graphmixer_backward: d_proj_w needs x0");
  for (int l = 0; l < a->num_layers; ++l) {
    const tgmx_mixer_layer_t& ly = a->layers[l];
    TGMX_REQUIRE(ly.tok_g && ly.tok_b && ly.ch_g && ly.ch_b && ly.ch_w1 && ly.ch_b1 && a->ch_w1T[l] && a->ch_w2T[l] &&
                     (ly.tok_hidden == 0 || (ly.tok_w1 && ly.tok_b1 && ly.tok_w2)),
                 "graphmixer_backward: layer %d's weights or their transposes are missing", l);
    if (!tgmx_mixer_train_supported(a->K, a->D, ly.tok_hidden)) {
      set_error("graphmixer_backward: layer %d's token block (K=%d, D=%d, hidden %d) does not fit the token kernels' LDS", l, a->K, a->D, ly.tok_hidden);
      return TGMX_E_UNSUPPORTED;
    }
  }
  size_t need = 0;
  if ((rc = gm_backward_pass(a, true, &need, nullptr))) return rc;
  TGMX_REQUIRE(a->workspace && a->workspace_bytes >= need, "graphmixer_backward: workspace too small (%zu bytes, %zu needed)", a->workspace_bytes, need);
  return gm_backward_pass(a, false, &need, stream);
}
