// TPNet training: the backward of tgmx_tpnet_forward_train (csrc/tpnet.hip) as one call, and its pieces.
//
//   tgmx_tpnet_token_backward   the token block with the forward's refined column mean: one workgroup per sequence, one thread per channel;
//                               writes dx and, per SEQUENCE, one row of partial sums of the six parameter gradients (no per-column rows)
//   tgmx_tpnet_mean_backward    the unmasked token mean
//   tgmx_tpnet_time_backward    the rows whose column sums are d time_encoder.w.{weight, bias}
//   tgmx_tpnet_backward         the whole chain; the channel block is csrc/mixer_bwd.hip's (mixer_channel_backward), the GEMMs and reductions
//                               are the dense library's (tgmx_sgemm_nt_ep, tgmx_sgemm_tn, tgmx_colsum, tgmx_relu_mask)
//
// No float atomics anywhere: every sum has a fixed order.
#include <math.h>

#include "common.h"
#include "edge_csr.h"

namespace tgmx {

__device__ __forceinline__ float tp_gelu_fwd(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }
__device__ __forceinline__ float tp_gelu_grad(float v) {
  return 0.5f * (1.f + erff(v * 0.70710678118654752f)) + v * 0.3989422804014327f * expf(-0.5f * v * v);
}

// ---- token block ------------------------------------------------------------------------------------------------------------------------------
// The compute phase is mixer_token_backward_kernel's (csrc/mixer_bwd.hip) with the refined mean: a chunk of kThreads channels, the column's
// 4 K + 2 Ht values in LDS at [feature][thread], pitch kThreads + 1.  Then, instead of writing the chunk's columns out, the workgroup sums
// them: thread t owns entries t, t + kThreads, ... of the partial row and walks the chunk's columns in ascending order, one FMA each,
// carrying the sums in registers from chunk to chunk -- channels ascending over the whole sequence, whatever the chunk width.  A wave reads
// one column at a time: the lanes' entries differ in the feature, features are kThreads + 1 floats apart, so the reads spread over the banks
// (lanes that share a feature read the same address).
template <int kThreads>
__global__ __launch_bounds__(kThreads) void tpnet_token_backward_kernel(
    const float* __restrict__ x, long long ldx, const float* __restrict__ dz1, long long ldd, int K, int C, const float* __restrict__ tg,
    const float* __restrict__ tbeta, const float* __restrict__ w1, const float* __restrict__ b1, int Ht, const float* __restrict__ w2, float eps,
    float* __restrict__ dx, long long ldo, float* __restrict__ part, long long ldp, const DropoutArgs d0, const DropoutArgs d1) {
  extern __shared__ float lds[];
  constexpr int P = kThreads + 1;
  float* __restrict__ DO = lds;                  // [K]: the output gradient, dropped
  float* __restrict__ XN = DO + (size_t)K * P;   // [K]: the LayerNorm's output
  float* __restrict__ DXN = XN + (size_t)K * P;  // [K]: its gradient
  float* __restrict__ XH = DXN + (size_t)K * P;  // [K]: x, then x-hat, then dxn x-hat
  float* __restrict__ HD = XH + (size_t)K * P;   // [Ht]: the hidden activations, dropped
  float* __restrict__ DA = HD + (size_t)Ht * P;  // [Ht]: the gradient at the pre-activations
  const long long s = blockIdx.x;
  const int t = threadIdx.x;
  const float* __restrict__ xs = x + s * K * ldx;
  const float* __restrict__ ds = dz1 + s * K * ldd;
  float* __restrict__ os = dx + s * K * ldo;
  const float invK = 1.f / (float)K;

  // this thread's entries of [ do^T hd | da^T xn | sum do | sum dxn | sum dxn xhat | sum da ]: the LDS rows of the two factors (fb < 0: a plain sum)
  const int KH = K * Ht, np = 2 * KH + 3 * K + Ht;
  const int nper = part ? (np + kThreads - 1) / kThreads : 0;
  float acc[kTpTokAcc];
  int fa[kTpTokAcc], fb[kTpTokAcc];
#pragma unroll
  for (int i = 0; i < kTpTokAcc; ++i) {
    const int e = t + i * kThreads;
    acc[i] = 0.f;
    int a = 0, b = -1;
    if (e < KH) {
      a = e / Ht, b = 4 * K + e % Ht;  // DO[k] HD[j]
    } else if (e < 2 * KH) {
      a = 4 * K + Ht + (e - KH) / K, b = K + (e - KH) % K;  // DA[j] XN[k]
    } else if (e < 2 * KH + K) {
      a = e - 2 * KH;  // DO
    } else if (e < 2 * KH + 2 * K) {
      a = 2 * K + (e - 2 * KH - K);  // DXN
    } else if (e < 2 * KH + 3 * K) {
      a = 3 * K + (e - 2 * KH - 2 * K);  // dxn x-hat
    } else if (e < np) {
      a = 4 * K + Ht + (e - 2 * KH - 3 * K);  // DA
    }
    fa[i] = a * P;
    fb[i] = b < 0 ? -1 : b * P;
  }

  for (int c0 = 0; c0 < C; c0 += kThreads) {
    const int c = c0 + t;
    if (c < C) {
      const unsigned long long col = (unsigned long long)s * C + c;
#pragma unroll 8
      for (int k = 0; k < K; ++k) XH[k * P + t] = xs[k * ldx + c];
#pragma unroll 8
      for (int k = 0; k < K; ++k) DO[k * P + t] = ds[k * ldd + c];
      // the forward's LayerNorm over the K tokens: the refined mean, the same three passes as mixer_token_kernel<true, .>
      float sum = 0.f;
      for (int k = 0; k < K; ++k) sum += XH[k * P + t];
      float mean = sum / (float)K;
      float rest = 0.f;
      for (int k = 0; k < K; ++k) rest += XH[k * P + t] - mean;
      mean += rest / (float)K;
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
        HD[j * P + t] = tp_gelu_fwd(a) * m;
        DA[j * P + t] = dh * m * tp_gelu_grad(a);
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
        os[k * ldo + c] = rstd * (dxn * tg[k] - m1 - xh * m2) + ds[k * ldd + c];
        XH[k * P + t] = dxn * xh;
      }
    }
    if (part) {  // (uniform over the workgroup)
      __syncthreads();
      const int n = C - c0 < kThreads ? C - c0 : kThreads;
      // columns outermost, the thread's entries in groups of kGroup independent FMA chains: the LDS reads of a group are in flight together
      // (an entry's own order stays columns ascending).  A group's entries past the row's end read row 0 and are never stored.
      constexpr int kGroup = 6;
      static_assert(kTpTokAcc % kGroup == 0, "whole groups");
#pragma unroll
      for (int i0 = 0; i0 < kTpTokAcc; i0 += kGroup) {
        if (i0 < nper) {
#pragma unroll 2
          for (int r = 0; r < n; ++r) {
#pragma unroll
            for (int i = i0; i < i0 + kGroup; ++i) {
              const float va = lds[fa[i] + r];
              const float vb = lds[(fb[i] < 0 ? fa[i] : fb[i]) + r];
              acc[i] = __fmaf_rn(va, fb[i] < 0 ? 1.f : vb, acc[i]);
            }
          }
        }
      }
      __syncthreads();
    }
  }
  if (part) {
    float* __restrict__ po = part + s * ldp;
#pragma unroll
    for (int i = 0; i < kTpTokAcc; ++i) {
      const int e = t + i * kThreads;
      if (i < nper && e < np) po[e] = acc[i];
    }
    for (long long e = np + t; e < ldp; e += kThreads) po[e] = 0.f;
  }
}

// ---- the small pieces ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tpnet_mean_backward_kernel(const float* __restrict__ g, long long ldg, long long R, int k, int C,
                                                                 float* __restrict__ dz, long long ldz) {
  const long long total = R * C;
  const long long step = (long long)gridDim.x * blockDim.x;
  const float fk = (float)k;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
    const long long r = e / C;
    const int c = (int)(e - r * C);
    dz[r * ldz + c] = g[(r / k) * ldg + c] / fk;
  }
}

__global__ __launch_bounds__(256) void tpnet_time_backward_kernel(const float* __restrict__ dtime, long long ldt, const double* __restrict__ lg,
                                                                 long long R, const float* __restrict__ tw, const float* __restrict__ tb, int dT,
                                                                 float* __restrict__ rows) {
  const long long total = R * dT;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
    const long long r = e / dT;
    const int c = (int)(e - r * dT);
    const double l = lg[r];
    float gw = 0.f, gb = 0.f;
    if (!(l < 0.0)) {  // (a pad row carries -1)
      const double v = -sin(fma((double)tw[c], l, (double)tb[c])) * (double)dtime[r * ldt + c];
      gw = (float)(v * l);
      gb = (float)v;
    }
    rows[r * 2 * dT + c] = gw;
    rows[r * 2 * dT + dT + c] = gb;
  }
}

static unsigned tp_blocks(long long total) {
  long long blocks = (total + 255) / 256;
  return (unsigned)(blocks > 16384 ? 16384 : (blocks < 1 ? 1 : blocks));
}

static bool tp_drop_ok(const tgmx_dropout_t* d) { return !d || (d->p >= 0.f && d->p < 1.f); }
static int64_t tp_up4(int64_t x) { return (x + 3) / 4 * 4; }

}  // namespace tgmx

using namespace tgmx;

extern "C" int tgmx_tpnet_train_supported(int32_t K, int32_t C, int32_t Ht) {
  if (K <= 0 || C <= 0 || Ht < 0 || K > 4096 || Ht > 4096) return 0;
  if (mixer_token_lds_bytes(K, C, Ht) > kMixerTokMaxLds) return 0;
  const int threads = mixer_token_bwd_threads(K, Ht);
  return threads > 0 && tpnet_token_part_floats(K, Ht) <= kTpTokAcc * threads ? 1 : 0;
}

extern "C" int tgmx_tpnet_token_backward(const float* x, int64_t ldx, const float* dz1, int64_t ldd, int64_t Q, int32_t K, int32_t C,
                                         const float* tok_g, const float* tok_b, const float* w1, const float* b1, int32_t Ht, const float* w2,
                                         float eps, float* dx, int64_t ldo, float* part, int64_t ldp, const tgmx_dropout_t* drop_hidden,
                                         const tgmx_dropout_t* drop_out, tgmx_stream_t stream) {
  TGMX_REQUIRE(Q >= 0 && Q < (1ll << 31) && K > 0 && C > 0 && Ht >= 0 && ldx >= C && ldd >= C && ldo >= C,
               "tpnet_token_backward: bad sizes Q=%lld K=%d C=%d Ht=%d", (long long)Q, K, C, Ht);
  TGMX_REQUIRE(tp_drop_ok(drop_hidden) && tp_drop_ok(drop_out), "tpnet_token_backward: p must be in [0, 1)");
  if (!tgmx_tpnet_train_supported(K, C, Ht)) {
    set_error("tpnet_token_backward: K=%d tokens x C=%d channels (token hidden %d) are outside the token kernels' envelope (64 KiB of LDS, a partial "
              "row of at most %d floats a thread)", K, C, Ht, kTpTokAcc);
    return TGMX_E_UNSUPPORTED;
  }
  TGMX_REQUIRE(!part || ldp >= tpnet_token_part_floats(K, Ht), "tpnet_token_backward: part rows of %lld floats, %d needed", (long long)ldp,
               tpnet_token_part_floats(K, Ht));
  if (Q == 0) return TGMX_OK;
  TGMX_REQUIRE(x && dz1 && dx && dx != dz1 && tok_g && tok_b && (Ht == 0 || (w1 && b1 && w2)), "tpnet_token_backward: null or aliased pointer");
  const int threads = mixer_token_bwd_threads(K, Ht);
  const size_t lds = mixer_token_bwd_lds_bytes(K, Ht, threads);
  const DropoutArgs d0 = make_dropout(drop_hidden), d1 = make_dropout(drop_out);
#define TGMX_TP_TOKEN_BWD(T)                                                                                                                     \
  hipLaunchKernelGGL(tpnet_token_backward_kernel<T>, dim3((unsigned)Q), dim3(T), lds, (hipStream_t)stream, x, (long long)ldx, dz1, (long long)ldd, \
                     K, C, tok_g, tok_b, w1, b1, Ht, w2, eps, dx, (long long)ldo, part, (long long)ldp, d0, d1)
  if (threads == 128) TGMX_TP_TOKEN_BWD(128);
  else if (threads == 64) TGMX_TP_TOKEN_BWD(64);
  else TGMX_TP_TOKEN_BWD(32);
#undef TGMX_TP_TOKEN_BWD
  TGMX_CHECK_LAUNCH("tpnet_token_backward");
  return TGMX_OK;
}

extern "C" int tgmx_tpnet_mean_backward(const float* g, int64_t ldg, int64_t Q, int32_t k, int32_t C, float* dz, int64_t ldz, tgmx_stream_t stream) {
  TGMX_REQUIRE(Q >= 0 && k > 0 && C > 0 && ldg >= C && ldz >= C && Q * k < (1ll << 40), "tpnet_mean_backward: bad sizes Q=%lld k=%d C=%d", (long long)Q, k, C);
  if (Q == 0) return TGMX_OK;
  TGMX_REQUIRE(g && dz, "tpnet_mean_backward: null pointer");
  hipLaunchKernelGGL(tpnet_mean_backward_kernel, dim3(tp_blocks((long long)Q * k * C)), dim3(256), 0, (hipStream_t)stream, g, (long long)ldg,
                     (long long)Q * k, k, C, dz, (long long)ldz);
  TGMX_CHECK_LAUNCH("tpnet_mean_backward");
  return TGMX_OK;
}

extern "C" int tgmx_tpnet_time_backward(const float* dtime, int64_t ldt, const double* lg, int64_t R, const float* tw, const float* tb, int32_t dT,
                                        float* rows, tgmx_stream_t stream) {
  TGMX_REQUIRE(R >= 0 && R < (1ll << 40) && dT > 0 && ldt >= dT, "tpnet_time_backward: bad sizes R=%lld dT=%d", (long long)R, dT);
  if (R == 0) return TGMX_OK;
  TGMX_REQUIRE(dtime && lg && tw && tb && rows, "tpnet_time_backward: null pointer");
  hipLaunchKernelGGL(tpnet_time_backward_kernel, dim3(tp_blocks((long long)R * dT)), dim3(256), 0, (hipStream_t)stream, dtime, (long long)ldt, lg,
                     (long long)R, tw, tb, dT, rows);
  TGMX_CHECK_LAUNCH("tpnet_time_backward");
  return TGMX_OK;
}

// ---- the whole backward as one call ---------------------------------------------------------------------------------------------------------
static bool tp_ch_wanted(const tgmx_mixer_layer_grad_t& d) { return d.ch_g || d.ch_b || d.ch_w1 || d.ch_b1 || d.ch_w2 || d.ch_b2; }

static int tp_bwd_check(const tgmx_tpnet_bwd_t* a, const char* what) {
  TGMX_REQUIRE(a, "%s: null argument block", what);
  TGMX_REQUIRE(a->B >= 0 && a->B < (1ll << 30) && a->k > 0 && a->dN >= 0 && a->dE >= 0 && a->dT >= 0 && a->E > 0 && a->od >= 0 && a->num_layers >= 0 &&
                   a->num_layers <= TGMX_MIXER_MAX_LAYERS && 2 * a->B * a->k * (long long)(a->E > a->od ? a->E : a->od) < (1ll << 38),
               "%s: bad sizes", what);
  const int W = a->dN + a->dT + a->dE + 2 * a->od;
  TGMX_REQUIRE(W > 0 && (a->B == 0 || (a->ldg >= a->E && a->ldx0 >= W && a->ldhp >= 2 * a->E && a->ldz >= a->E && (a->od == 0 || (a->ldf >= a->od && a->ldfh >= 4 * a->od)))),
               "%s: leading dimensions", what);
  TGMX_REQUIRE(a->drop_p >= 0.f && a->drop_p < 1.f, "%s: p must be in [0, 1)", what);
  for (int l = 0; l < a->num_layers; ++l)
    TGMX_REQUIRE(a->layers[l].ch_hidden > 0 && a->layers[l].tok_hidden >= 0 && (a->B == 0 || a->ldh >= a->layers[l].ch_hidden), "%s: layer %d's widths", what, l);
  return TGMX_OK;
}

// dry: lay the workspace out only (*need = its size), launch nothing
static int tp_backward_pass(const tgmx_tpnet_bwd_t* a, bool dry, size_t* need, tgmx_stream_t stream) {
  const int64_t Q = 2 * a->B, R = Q * a->k;
  const int K = a->k, E = a->E, L = a->num_layers, od = a->od, dT = a->dT;
  const int W = a->dN + dT + a->dE + 2 * od;
  const int64_t ldz = a->ldz, ldh = a->ldh, ldhp = a->ldhp, ldf = a->ldf, ldfh = a->ldfh, ldt = tp_up4(dT);
  const bool dropping = a->drop_p > 0.f;
  hipStream_t st = (hipStream_t)stream;
  // what is wanted, from the bottom of the chain up
  const bool want_rp1 = od > 0 && (a->d_rp_w1 || a->d_rp_b1), want_rp = od > 0 && (want_rp1 || a->d_rp_w2 || a->d_rp_b2);
  const bool want_time = dT > 0 && (a->d_tw || a->d_tb);
  const bool want_hp = a->d_proj_w0 || a->d_proj_b0 || want_rp || want_time;
  const bool want_proj = want_hp || a->d_proj_w2 || a->d_proj_b2;
  // lowest: the lowest layer whose token block's input gradient, or a gradient of its own, somebody reads (L: nobody's)
  int lowest = L;
  if (want_proj) lowest = 0;
  else
    for (int l = 0; l < L; ++l)
      if (a->d_tok[l] || tp_ch_wanted(a->d_layers[l])) {
        lowest = l;
        break;
      }
  const bool chain = want_proj || lowest < L;
  int Hc = 1, Ht = 0;
  for (int l = 0; l < L; ++l) {
    Hc = a->layers[l].ch_hidden > Hc ? a->layers[l].ch_hidden : Hc;
    Ht = a->layers[l].tok_hidden > Ht ? a->layers[l].tok_hidden : Ht;
  }
  const int np_max = tpnet_token_part_floats(K, Ht);
  const int64_t ldp = tp_up4(np_max);
  bool any_tok = false;
  for (int l = lowest; l < L; ++l) any_tok = any_tok || a->d_tok[l];

  WorkspaceCarver ws(dry ? nullptr : a->workspace);
  const size_t Rz = chain ? (size_t)R * ldz : 0, Rl = L > lowest ? Rz : 0, Rh = L > lowest ? (size_t)R * ldh : 0;
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
  float* part = ws.take<float>(any_tok ? (size_t)Q * ldp : 0);
  float* dhp = ws.take<float>(want_hp ? (size_t)R * ldhp : 0);
  float* dtime = ws.take<float>(want_time ? (size_t)R * ldt : 0);
  float* trows = ws.take<float>(want_time ? (size_t)R * 2 * dT : 0);
  float* dpf = ws.take<float>(want_rp ? (size_t)2 * R * ldf : 0);
  float* dfh = ws.take<float>(want_rp1 ? (size_t)2 * R * ldfh : 0);
  size_t tn_bytes = tgmx_sgemm_tn_workspace_bytes(R, E, 2 * E, 1);
  auto grow = [&](size_t b) { tn_bytes = b > tn_bytes ? b : tn_bytes; };
  grow(tgmx_sgemm_tn_workspace_bytes(R, 2 * E, W, 1));
  if (od > 0) {
    grow(tgmx_sgemm_tn_workspace_bytes(2 * R, od, 4 * od, 1));
    grow(tgmx_sgemm_tn_workspace_bytes(2 * R, 4 * od, od, 1));
  }
  for (int l = lowest; l < L; ++l) {
    grow(tgmx_sgemm_tn_workspace_bytes(R, E, a->layers[l].ch_hidden, 1));
    grow(tgmx_sgemm_tn_workspace_bytes(R, a->layers[l].ch_hidden, E, 1));
  }
  float* tn_ws = ws.take<float>(tn_bytes / sizeof(float) + 1);
  int widest = 2 * E > Hc ? 2 * E : Hc;
  widest = np_max > widest ? np_max : widest;
  widest = 4 * od > widest ? 4 * od : widest;
  widest = dT > widest ? dT : widest;
  float* cs_ws = ws.take<float>((size_t)256 * widest);
  *need = ws.total();
  if (dry || !chain) return TGMX_OK;

  int rc;
  // 1. the token mean
  if ((rc = tgmx_tpnet_mean_backward(a->g, a->ldg, Q, K, E, gz, ldz, stream))) return rc;
  // 2. the layers, last first
  if (L > lowest && hipMemsetAsync(zero, 0, (size_t)ldz * sizeof(float), st) != hipSuccess) {
    set_error("tpnet_backward: hipMemsetAsync failed");
    return TGMX_E_LAUNCH;
  }
  const size_t per = (size_t)R * ldz;
  const MixerChannelBufs cb{abuf, hbuf, y, dy, du, dgx, gt, zero, tn_ws, cs_ws};
  for (int l = L - 1; l >= lowest; --l) {
    const tgmx_mixer_layer_t& ly = a->layers[l];
    const int ht = ly.tok_hidden;
    const bool tok = a->d_tok[l] != nullptr, down = tok || l > lowest || want_proj;  // somebody reads dz1
    tgmx_dropout_t site[4];
    for (int s = 0; s < 4; ++s) site[s] = tgmx_dropout_t{a->drop_p, a->drop_seed, a->drop_stream + 4ull * l + s, 0};
    if ((rc = mixer_channel_backward(ly, a->d_layers[l], a->ch_w1T[l], a->ch_w2T[l], a->save_z1 + l * per, gz, R, E, ldz, ldh, a->eps, site, down, cb,
                                     stream)))
      return rc;
    if (!down) return TGMX_OK;
    if ((rc = tgmx_tpnet_token_backward(a->save_z + l * per, ldz, du, ldz, Q, K, E, ly.tok_g, ly.tok_b, ly.tok_w1, ly.tok_b1, ht, ly.tok_w2, a->eps, gz2,
                                        ldz, tok ? part : nullptr, ldp, &site[0], &site[1], stream)))
      return rc;
    if (tok && (rc = tgmx_colsum(part, ldp, Q, tpnet_token_part_floats(K, ht), a->d_tok[l], 0, cs_ws, stream))) return rc;
    float* tmp = gz;
    gz = gz2;
    gz2 = tmp;
  }
  if (!want_proj) return TGMX_OK;
  // 3. the projection
  if (a->d_proj_w2 && (rc = tgmx_sgemm_tn(gz, ldz, a->hp, ldhp, a->d_proj_w2, 2 * E, R, E, 2 * E, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
  if (a->d_proj_b2 && (rc = tgmx_colsum(gz, ldz, R, E, a->d_proj_b2, 0, cs_ws, stream))) return rc;
  if (!want_hp) return TGMX_OK;
  if ((rc = tgmx_sgemm_nt_ep(gz, ldz, a->proj_w2T, E, dhp, ldhp, R, 2 * E, E, nullptr, 0, nullptr, 0, stream))) return rc;
  if ((rc = tgmx_relu_mask(dhp, ldhp, a->hp, ldhp, R, 2 * E, stream))) return rc;
  if (a->d_proj_w0 && (rc = tgmx_sgemm_tn(dhp, ldhp, a->x0, a->ldx0, a->d_proj_w0, W, R, 2 * E, W, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
  if (a->d_proj_b0 && (rc = tgmx_colsum(dhp, ldhp, R, 2 * E, a->d_proj_b0, 0, cs_ws, stream))) return rc;
  // 4. the time encoder: only the dT time columns of dx0 are formed
  if (want_time) {
    if ((rc = tgmx_sgemm_nt_ep(dhp, ldhp, a->w0T_time, 2 * E, dtime, ldt, R, dT, 2 * E, nullptr, 0, nullptr, 0, stream))) return rc;
    if ((rc = tgmx_tpnet_time_backward(dtime, ldt, a->lg, R, a->tw, a->tb, dT, trows, stream))) return rc;
    if (a->d_tw && (rc = tgmx_colsum(trows, 2 * dT, R, dT, a->d_tw, 0, cs_ws, stream))) return rc;
    if (a->d_tb && (rc = tgmx_colsum(trows + dT, 2 * dT, R, dT, a->d_tb, 0, cs_ws, stream))) return rc;
  }
  // 5. the pair-feature MLP over the 2 R rows: the two pair blocks of dx0 go straight to dpf[0:R] and dpf[R:2R]
  if (want_rp) {
    if ((rc = tgmx_sgemm_nt_ep(dhp, ldhp, a->w0T_pair0, 2 * E, dpf, ldf, R, od, 2 * E, nullptr, 0, nullptr, 0, stream))) return rc;
    if ((rc = tgmx_sgemm_nt_ep(dhp, ldhp, a->w0T_pair1, 2 * E, dpf + (size_t)R * ldf, ldf, R, od, 2 * E, nullptr, 0, nullptr, 0, stream))) return rc;
    if (a->d_rp_w2 && (rc = tgmx_sgemm_tn(dpf, ldf, a->feat_h, ldfh, a->d_rp_w2, 4 * od, 2 * R, od, 4 * od, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
    if (a->d_rp_b2 && (rc = tgmx_colsum(dpf, ldf, 2 * R, od, a->d_rp_b2, 0, cs_ws, stream))) return rc;
    if (want_rp1) {
      if ((rc = tgmx_sgemm_nt_ep(dpf, ldf, a->rp_w2T, od, dfh, ldfh, 2 * R, 4 * od, od, nullptr, 0, nullptr, 0, stream))) return rc;
      if ((rc = tgmx_relu_mask(dfh, ldfh, a->feat_h, ldfh, 2 * R, 4 * od, stream))) return rc;
      if (a->d_rp_w1 && (rc = tgmx_sgemm_tn(dfh, ldfh, a->feat, ldf, a->d_rp_w1, od, 2 * R, 4 * od, od, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
      if (a->d_rp_b1 && (rc = tgmx_colsum(dfh, ldfh, 2 * R, 4 * od, a->d_rp_b1, 0, cs_ws, stream))) return rc;
    }
  }
  return TGMX_OK;
}

extern "C" size_t tgmx_tpnet_backward_workspace_bytes(const tgmx_tpnet_bwd_t* a) {
  size_t need = 0;
  if (tp_bwd_check(a, "tpnet_backward_workspace_bytes") != TGMX_OK) return 0;
  return tp_backward_pass(a, true, &need, nullptr) == TGMX_OK ? need : 0;
}

extern "C" int tgmx_tpnet_backward(const tgmx_tpnet_bwd_t* a, tgmx_stream_t stream) {
  int rc;
  if ((rc = tp_bwd_check(a, "tpnet_backward"))) return rc;
  if (a->B == 0) return TGMX_OK;
  TGMX_REQUIRE(a->g, "tpnet_backward: the upstream gradient is missing");
  TGMX_REQUIRE(a->num_layers == 0 || (a->save_z && a->save_z1), "tpnet_backward: the layers' saved inputs are missing");
  const bool want_rp = a->od > 0 && (a->d_rp_w1 || a->d_rp_b1 || a->d_rp_w2 || a->d_rp_b2), want_time = a->dT > 0 && (a->d_tw || a->d_tb);
  const bool want_hp = a->d_proj_w0 || a->d_proj_b0 || want_rp || want_time;
  TGMX_REQUIRE(!(want_hp || a->d_proj_w2) || a->hp, "tpnet_backward: the projection's gradients need hp");
  TGMX_REQUIRE(!want_hp || a->proj_w2T, "tpnet_backward: proj_w2T is missing");
  TGMX_REQUIRE(!a->d_proj_w0 || a->x0, "tpnet_backward: d_proj_w0 needs x0");
  TGMX_REQUIRE(!want_time || (a->lg && a->tw && a->tb && a->w0T_time), "tpnet_backward: the time encoder's gradients need lg, tw, tb and w0T_time");
  TGMX_REQUIRE(!want_rp || (a->feat && a->feat_h && a->w0T_pair0 && a->w0T_pair1 && a->rp_w2T),
               "tpnet_backward: the pair-feature MLP's gradients need feat, feat_h, w0T_pair0 / w0T_pair1 and rp_w2T");
  for (int l = 0; l < a->num_layers; ++l) {
    const tgmx_mixer_layer_t& ly = a->layers[l];
    TGMX_REQUIRE(ly.tok_g && ly.tok_b && ly.ch_g && ly.ch_b && ly.ch_w1 && ly.ch_b1 && a->ch_w1T[l] && a->ch_w2T[l] &&
                     (ly.tok_hidden == 0 || (ly.tok_w1 && ly.tok_b1 && ly.tok_w2)),
                 "tpnet_backward: layer %d's weights or their transposes are missing", l);
    if (!tgmx_tpnet_train_supported(a->k, a->E, ly.tok_hidden)) {
      set_error("tpnet_backward: layer %d's token block (k=%d, E=%d, hidden %d) is outside the token kernels' envelope", l, a->k, a->E, ly.tok_hidden);
      return TGMX_E_UNSUPPORTED;
    }
  }
  size_t need = 0;
  if ((rc = tp_backward_pass(a, true, &need, nullptr))) return rc;
  TGMX_REQUIRE(a->workspace && a->workspace_bytes >= need, "tpnet_backward: workspace too small (%zu bytes, %zu needed)", a->workspace_bytes, need);
  return tp_backward_pass(a, false, &need, stream);
}
