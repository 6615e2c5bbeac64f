// GraphMixer (the reference's examples/linkproppred/graphmixer.py) for gfx950: the time-gap neighbour grouping of its hook and the
// inference forward of its encoder -- Time2Vec prologue, MLPMixer token mixing (with the next channel LayerNorm fused in), the tail
// (masked mean over the sampled slots, time-gap node encoder, concatenation).  The dense contractions (projection, channel FFNs, output
// layer) run on the exact-fp32 MFMA GEMM of csrc/dense.hip through tgmx_sgemm_nt_ep (GELU / residual epilogues).  The same launches with
// per-call buffers and the layers' dropout sites are the training forward (tgmx_graphmixer_forward_train); its backward is csrc/mixer_bwd.hip.
#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

namespace tgmx {

// ---- time-gap grouping ------------------------------------------------------------------------------------------------------------

// incidence 2j = (u_j -> v_j), 2j + 1 = (v_j -> u_j): a stable sort by key keeps every node's neighbours in stream order
__global__ __launch_bounds__(256) void tg_interleave_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ dst, long long W,
                                                           int32_t* __restrict__ keys, int32_t* __restrict__ vals) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= W) return;
  const int32_t u = src[j], v = dst[j];
  keys[2 * j] = u;
  vals[2 * j] = v;
  keys[2 * j + 1] = v;
  vals[2 * j + 1] = u;
}

__device__ __forceinline__ int32_t seed_at(const int32_t* s0, long long n0, const int32_t* s1, long long n1, const int32_t* s2, long long i) {
  return i < n0 ? s0[i] : (i < n0 + n1 ? s1[i - n0] : s2[i - n0 - n1]);
}

// each seed's run [lower_bound, upper_bound) in the sorted keys (n == 0: every run empty)
__global__ __launch_bounds__(256) void tg_lookup_kernel(const int32_t* __restrict__ sorted, long long n, const int32_t* s0, long long n0,
                                                       const int32_t* s1, long long n1, const int32_t* s2, long long S,
                                                       int32_t* __restrict__ out_lo, int32_t* __restrict__ out_cnt) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S) return;
  const int32_t v = seed_at(s0, n0, s1, n1, s2, i);
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (sorted[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  long long up = lo, hi2 = n;
  while (up < hi2) {
    const long long mid = (up + hi2) >> 1;
    if (sorted[mid] <= v) up = mid + 1;
    else hi2 = mid;
  }
  out_lo[i] = (int32_t)lo;
  out_cnt[i] = (int32_t)(up - lo);
}

static size_t tg_sort_temp_bytes(long long n) {
  size_t tb = 0;
  (void)rocprim::radix_sort_pairs(nullptr, tb, (const int*)nullptr, (int*)nullptr, (const int*)nullptr, (int*)nullptr, (size_t)n, 0u, 32u);
  return tb;
}

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- link-encoder prologue ----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void mixer_prologue_kernel(const float* __restrict__ ex, const int64_t* __restrict__ seed_t,
                                                            const int64_t* __restrict__ nbr_t, long long R, int K, int D,
                                                            const float* __restrict__ tw, const float* __restrict__ tb, int T,
                                                            float* __restrict__ out, long long ldo) {
  const long long total = R * ldo;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
    const long long r = e / ldo;
    const int c = (int)(e - r * ldo);
    float v = 0.f;
    if (c < D) {
      v = ex[r * D + c];
    } else if (c < D + T) {
      const float dt = (float)(seed_t[r / K] - nbr_t[r]);  // int64 difference, then .float() (Time2Vec.forward)
      v = cosf(__fmaf_rn(dt, tw[c - D], tb[c - D]));
    }
    out[e] = v;
  }
}

// ---- token mixing --------------------------------------------------------------------------------------------------------------------
// One workgroup per seed.  Pass 1, one thread per channel (chunks of kTokThreads): LayerNorm over the K tokens of the channel's column,
// the two small Linears with GELU between them, the residual -> z1 tile [K][C] in LDS.  Pass 2, one wave per token: LayerNorm over the
// C channels of the z1 row -> z1 and y rows in global memory.
constexpr int kTokThreads = kMixerTokThreads;
constexpr size_t kTokMaxLds = kMixerTokMaxLds;

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }

// kRefine (TPNet): one correction step on the column mean, mean += sum(x - mean) / K.  The K tokens of an all-pad TPNet sequence are identical,
// so the column is constant; an error d in its mean leaves the LayerNorm as d / sqrt(eps) = 316 d where the exact answer is 0.  With the
// correction the mean of K equal values is that value, bit for bit.  GraphMixer keeps the plain mean (its results stay as they were).
// kDrop (training): the counter-based dropout of common.h after the GELU (element (s C + c) Ht + j of stream d0) and on the block's output
// before the residual (element (s C + c) K + k of stream d1); without it the arithmetic is the inference kernel's, expression for expression.
template <bool kRefine, bool kDrop>
__global__ __launch_bounds__(kTokThreads) void mixer_token_kernel(const float* __restrict__ x, long long ldx, int K, int C,
                                                                  const float* __restrict__ tg, const float* __restrict__ tbeta,
                                                                  const float* __restrict__ w1, const float* __restrict__ b1, int Ht,
                                                                  const float* __restrict__ w2, const float* __restrict__ b2,
                                                                  const float* __restrict__ cg, const float* __restrict__ cb, float eps,
                                                                  float* __restrict__ z1, float* __restrict__ y, long long ldo,
                                                                  const DropoutArgs d0, const DropoutArgs d1) {
  extern __shared__ float lds[];
  float* __restrict__ zt = lds;                         // [K][C]: the seed's z1 tile
  float* __restrict__ xn = lds + (size_t)K * C;         // [K][kTokThreads]: the normalised column of each thread
  float* __restrict__ hb = xn + (size_t)K * kTokThreads;  // [Ht][kTokThreads]: its hidden activations
  const long long s = blockIdx.x;
  const int t = threadIdx.x;
  const float* __restrict__ xs = x + s * K * ldx;
  for (int c0 = 0; c0 < C; c0 += kTokThreads) {
    const int c = c0 + t;
    if (c < C) {
      // the column is read from global memory ONCE, all K loads in flight together (a loop that adds each load as it arrives waits
      // out one memory latency per token); it stays in the z1 tile for the residual
#pragma unroll 8
      for (int k = 0; k < K; ++k) zt[k * C + c] = xs[k * ldx + c];
      float sum = 0.f;
      for (int k = 0; k < K; ++k) sum += zt[k * C + c];
      float mean = sum / (float)K;
      if constexpr (kRefine) {
        float rest = 0.f;
        for (int k = 0; k < K; ++k) rest += zt[k * C + c] - mean;
        mean += rest / (float)K;
      }
      float var = 0.f;
      for (int k = 0; k < K; ++k) {
        const float d = zt[k * C + c] - mean;
        var = __fmaf_rn(d, d, var);
      }
      const float rstd = 1.f / sqrtf(var / (float)K + eps);
      for (int k = 0; k < K; ++k) xn[k * kTokThreads + t] = (zt[k * C + c] - mean) * rstd * tg[k] + tbeta[k];
      [[maybe_unused]] const unsigned long long col = (unsigned long long)s * C + c;
      for (int j = 0; j < Ht; ++j) {
        float a = 0.f;
        for (int k = 0; k < K; ++k) a = __fmaf_rn(w1[j * K + k], xn[k * kTokThreads + t], a);
        if constexpr (kDrop) hb[j * kTokThreads + t] = gelu_erf(a + b1[j]) * dropout_scale(d0, col * Ht + j);
        else hb[j * kTokThreads + t] = gelu_erf(a + b1[j]);
      }
      for (int k = 0; k < K; ++k) {
        float a = 0.f;
        for (int j = 0; j < Ht; ++j) a = __fmaf_rn(w2[k * Ht + j], hb[j * kTokThreads + t], a);
        if constexpr (kDrop) zt[k * C + c] += (a + b2[k]) * dropout_scale(d1, col * K + k);
        else zt[k * C + c] += a + b2[k];
      }
    }
  }
  __syncthreads();
  const int lane = t & (kWave - 1), wave = t / kWave;
  constexpr int kWaves = kTokThreads / kWave;
  for (int k = wave; k < K; k += kWaves) {
    const float* __restrict__ row = zt + (size_t)k * C;
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
    float* __restrict__ zo = z1 + (s * K + k) * ldo;
    float* __restrict__ yo = y + (s * K + k) * ldo;
    for (int c = lane; c < C; c += kWave) {
      const float v = row[c];
      zo[c] = v;
      yo[c] = (v - mean) * rstd * cg[c] + cb[c];
    }
  }
}

static size_t token_lds_bytes(int K, int C, int Ht) { return mixer_token_lds_bytes(K, C, Ht); }

// ---- tail ----------------------------------------------------------------------------------------------------------------------------

// one workgroup (kTailWaves waves) per seed: the link mean with every slot's load in flight together; the time-gap run split over the
// waves (wave w sums entries w, w + kTailWaves, ...; the partial sums meet in LDS in wave order: deterministic) -- a hub seed's run is
// hundreds of entries long
constexpr int kTailWaves = 4;

__global__ __launch_bounds__(kTailWaves * kWave) void mixer_tail_kernel(const float* __restrict__ z, long long ldz, int K, int C,
                                                                        const int32_t* __restrict__ nbr_nids, const float* __restrict__ node_x,
                                                                        int F, const int32_t* __restrict__ tg_nbr,
                                                                        const int32_t* __restrict__ tg_lo, const int32_t* __restrict__ tg_cnt,
                                                                        const int32_t* s0, long long n0, const int32_t* s1, long long n1,
                                                                        const int32_t* s2, float* __restrict__ out, long long ldo) {
  __shared__ float part[kTailWaves][kWave];
  const long long i = blockIdx.x;
  const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
  int valid = 0;
  for (int k = 0; k < K; ++k) valid += nbr_nids[i * K + k] != -1;
  const float denom = (float)(valid > 0 ? valid : 1);
  float* __restrict__ o = out + i * ldo;
  const float* __restrict__ zs = z + i * K * ldz;
  for (int c = t; c < C; c += blockDim.x) {
    float a = 0.f;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      const float v = zs[k * ldz + c];
      a += nbr_nids[i * K + k] != -1 ? v : 0.f;
    }
    o[c] = a / denom;
  }
  const int lo = tg_lo[i], cnt = tg_cnt[i];
  const long long seed = seed_at(s0, n0, s1, n1, s2, i);
  for (int f0 = 0; f0 < F; f0 += kWave) {
    const int f = f0 + lane;
    float a = 0.f;
    if (f < F) {
#pragma unroll 4
      for (int j = wave; j < cnt; j += kTailWaves) a += node_x[(long long)tg_nbr[lo + j] * F + f];
    }
    part[wave][lane] = a;
    __syncthreads();
    if (wave == 0 && f < F) {
      float sum = part[0][lane];
#pragma unroll
      for (int w = 1; w < kTailWaves; ++w) sum += part[w][lane];
      o[C + f] = (cnt > 0 ? sum / (float)cnt : 0.f) + node_x[seed * F + f];
    }
    __syncthreads();
  }
  for (long long c = C + F + t; c < ldo; c += blockDim.x) o[c] = 0.f;
}

}  // namespace tgmx

using namespace tgmx;

extern "C" size_t tgmx_time_gap_workspace_bytes(int64_t W) {
  const long long n = W > 0 ? 2 * W : 1;
  return 3 * up256((size_t)n * 4) + up256(tg_sort_temp_bytes(n)) + 256;  // keys | vals | sorted keys | sort temp
}

extern "C" int tgmx_time_gap_group(const int32_t* src, const int32_t* dst, int64_t e_lo, int64_t W, const int32_t* seeds0, int64_t n0,
                                   const int32_t* seeds1, int64_t n1, const int32_t* seeds2, int64_t n2, void* workspace,
                                   size_t workspace_bytes, int32_t* out_nbr, int32_t* out_lo, int32_t* out_cnt, tgmx_stream_t stream) {
  TGMX_REQUIRE(W >= 0 && 2 * W < (1ll << 31) && e_lo >= 0 && n0 >= 0 && n1 >= 0 && n2 >= 0, "time_gap_group: bad sizes W=%lld", (long long)W);
  TGMX_REQUIRE((n0 == 0 || seeds0) && (n1 == 0 || seeds1) && (n2 == 0 || seeds2), "time_gap_group: null seed pointer");
  const long long S = n0 + n1 + n2, n = 2 * W;
  hipStream_t st = (hipStream_t)stream;
  const int32_t* sorted = nullptr;
  if (n > 0) {
    TGMX_REQUIRE(src && dst && out_nbr && workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= tgmx_time_gap_workspace_bytes(W),
                 "time_gap_group: null / misaligned / short workspace");
    char* base = reinterpret_cast<char*>(workspace);
    int32_t* keys = reinterpret_cast<int32_t*>(base);
    int32_t* vals = reinterpret_cast<int32_t*>(base + up256((size_t)n * 4));
    int32_t* skeys = reinterpret_cast<int32_t*>(base + 2 * up256((size_t)n * 4));
    void* temp = base + 3 * up256((size_t)n * 4);
    hipLaunchKernelGGL(tg_interleave_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, src + e_lo, dst + e_lo, (long long)W, keys, vals);
    TGMX_CHECK_LAUNCH("time_gap_group(interleave)");
    size_t tb = tg_sort_temp_bytes(n);
    if (rocprim::radix_sort_pairs(temp, tb, (const int*)keys, (int*)skeys, (const int*)vals, (int*)out_nbr, (size_t)n, 0u, 32u, st) != hipSuccess) {
      set_error("time_gap_group: rocprim::radix_sort_pairs failed");
      return TGMX_E_LAUNCH;
    }
    sorted = skeys;
  }
  if (S > 0) {
    TGMX_REQUIRE(out_lo && out_cnt, "time_gap_group: null output");
    hipLaunchKernelGGL(tg_lookup_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, sorted, n, seeds0, (long long)n0, seeds1,
                       (long long)n1, seeds2, S, out_lo, out_cnt);
    TGMX_CHECK_LAUNCH("time_gap_group(lookup)");
  }
  return TGMX_OK;
}

extern "C" int tgmx_mixer_prologue(const float* edge_x, const int64_t* seed_t, const int64_t* nbr_t, int64_t S, int32_t K, int32_t D,
                                   const float* tw, const float* tb, int32_t T, float* out, int64_t ldo, tgmx_stream_t stream) {
  TGMX_REQUIRE(S >= 0 && K > 0 && D >= 0 && T > 0 && ldo >= D + T, "mixer_prologue: bad sizes S=%lld K=%d D=%d T=%d", (long long)S, K, D, T);
  if (S == 0) return TGMX_OK;
  TGMX_REQUIRE((D == 0 || edge_x) && seed_t && nbr_t && tw && tb && out, "mixer_prologue: null pointer");
  const long long total = S * K * ldo;
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(mixer_prologue_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, edge_x, seed_t, nbr_t, (long long)S * K,
                     K, D, tw, tb, T, out, (long long)ldo);
  TGMX_CHECK_LAUNCH("mixer_prologue");
  return TGMX_OK;
}

static int mixer_token_run(bool refine, const float* x, int64_t ldx, int64_t S, int32_t K, int32_t C, const float* tok_g, const float* tok_b,
                           const float* w1, const float* b1, int32_t Ht, const float* w2, const float* b2, const float* ch_g, const float* ch_b,
                           float eps, float* z1, float* y, int64_t ldo, tgmx_stream_t stream, const tgmx_dropout_t* drop_hidden = nullptr,
                           const tgmx_dropout_t* drop_out = nullptr) {
  TGMX_REQUIRE(S >= 0 && K > 0 && C > 0 && Ht >= 0 && ldx >= C && ldo >= C, "mixer_token: bad sizes S=%lld K=%d C=%d Ht=%d", (long long)S, K, C, Ht);
  if (S == 0) return TGMX_OK;
  TGMX_REQUIRE(x && tok_g && tok_b && (Ht == 0 || (w1 && b1 && w2)) && b2 && ch_g && ch_b && z1 && y, "mixer_token: null pointer");
  const size_t lds = token_lds_bytes(K, C, Ht);
  if (lds > kTokMaxLds) {
    set_error("mixer_token: K=%d tokens x C=%d channels (token hidden %d) need %zu bytes of LDS per seed, more than %zu", K, C, Ht, lds, kTokMaxLds);
    return TGMX_E_UNSUPPORTED;
  }
  const DropoutArgs d0 = make_dropout(drop_hidden), d1 = make_dropout(drop_out);
  const bool drop = d0.thresh != 0 || d1.thresh != 0;
  if (refine && drop)
    hipLaunchKernelGGL((mixer_token_kernel<true, true>), dim3((unsigned)S), dim3(kTokThreads), lds, (hipStream_t)stream, x, (long long)ldx, K, C, tok_g,
                       tok_b, w1, b1, Ht, w2, b2, ch_g, ch_b, eps, z1, y, (long long)ldo, d0, d1);
  else if (refine)
    hipLaunchKernelGGL((mixer_token_kernel<true, false>), dim3((unsigned)S), dim3(kTokThreads), lds, (hipStream_t)stream, x, (long long)ldx, K, C, tok_g,
                       tok_b, w1, b1, Ht, w2, b2, ch_g, ch_b, eps, z1, y, (long long)ldo, d0, d1);
  else if (drop)
    hipLaunchKernelGGL((mixer_token_kernel<false, true>), dim3((unsigned)S), dim3(kTokThreads), lds, (hipStream_t)stream, x, (long long)ldx, K, C, tok_g,
                       tok_b, w1, b1, Ht, w2, b2, ch_g, ch_b, eps, z1, y, (long long)ldo, d0, d1);
  else
    hipLaunchKernelGGL((mixer_token_kernel<false, false>), dim3((unsigned)S), dim3(kTokThreads), lds, (hipStream_t)stream, x, (long long)ldx, K, C, tok_g,
                       tok_b, w1, b1, Ht, w2, b2, ch_g, ch_b, eps, z1, y, (long long)ldo, d0, d1);
  TGMX_CHECK_LAUNCH("mixer_token");
  return TGMX_OK;
}

int tgmx::mixer_layers_run(bool refine, const tgmx_mixer_layer_t* layers, int num_layers, int64_t S, int32_t K, int32_t C, float eps, float* z,
                           float* z1, float* y, int64_t ldz, float* h, int64_t ldh, tgmx_stream_t stream) {
  const long long R = (long long)S * K;
  int rc;
  for (int l = 0; l < num_layers; ++l) {
    const tgmx_mixer_layer_t& ly = layers[l];
    if ((rc = mixer_token_run(refine, z, ldz, S, K, C, ly.tok_g, ly.tok_b, ly.tok_w1, ly.tok_b1, ly.tok_hidden, ly.tok_w2, ly.tok_b2, ly.ch_g, ly.ch_b,
                              eps, z1, y, ldz, stream)))
      return rc;
    if ((rc = tgmx_sgemm_nt_ep(y, ldz, ly.ch_w1, C, h, ldh, R, ly.ch_hidden, C, ly.ch_b1, 2, nullptr, 0, stream))) return rc;
    if ((rc = tgmx_sgemm_nt_ep(h, ldh, ly.ch_w2, ly.ch_hidden, z, ldz, R, C, ly.ch_hidden, ly.ch_b2, 0, z1, ldz, stream))) return rc;
  }
  return TGMX_OK;
}

// the saving form of mixer_layers_run (training): layer l reads its input from save_z + l R ldz, leaves its token block's output in
// save_z1 + l R ldz and writes its output to layer l + 1's input, the last one to z_last.  drop: the sites' common descriptor (site s of
// layer l draws from stream + 4 l + s), NULL or p = 0 = off -- then the launches are mixer_layers_run's, writing elsewhere.
int tgmx::mixer_layers_run_train(bool refine, const tgmx_mixer_layer_t* layers, int num_layers, int64_t S, int32_t K, int32_t C, float eps,
                                 float* save_z, float* save_z1, float* z_last, float* y, int64_t ldz, float* h, int64_t ldh,
                                 const tgmx_dropout_t* drop, tgmx_stream_t stream) {
  const long long R = (long long)S * K;
  const int L = num_layers;
  const bool dropping = drop && drop->p > 0.f;
  const size_t per = (size_t)R * ldz;
  float* z_in = save_z;
  int rc;
  for (int l = 0; l < L; ++l) {
    const tgmx_mixer_layer_t& ly = layers[l];
    float* z1 = save_z1 + l * per;
    float* z_out = l + 1 < L ? save_z + (l + 1) * per : z_last;
    tgmx_dropout_t site[4];
    for (int s = 0; s < 4; ++s) {
      site[s].p = dropping ? drop->p : 0.f;
      site[s].seed = dropping ? drop->seed : 0;
      site[s].stream = dropping ? drop->stream + 4ull * l + s : 0;
      site[s].row0 = 0;
    }
    if ((rc = mixer_token_run(refine, z_in, ldz, S, K, C, ly.tok_g, ly.tok_b, ly.tok_w1, ly.tok_b1, ly.tok_hidden, ly.tok_w2, ly.tok_b2, ly.ch_g, ly.ch_b,
                              eps, z1, y, ldz, stream, &site[0], &site[1])))
      return rc;
    if ((rc = tgmx_sgemm_nt_ep(y, ldz, ly.ch_w1, C, h, ldh, R, ly.ch_hidden, C, ly.ch_b1, 2, nullptr, 0, stream))) return rc;
    if (!dropping) {
      if ((rc = tgmx_sgemm_nt_ep(h, ldh, ly.ch_w2, ly.ch_hidden, z_out, ldz, R, C, ly.ch_hidden, ly.ch_b2, 0, z1, ldz, stream))) return rc;
    } else {
      if ((rc = tgmx_dropout(h, ldh, R, ly.ch_hidden, &site[2], h, ldh, stream))) return rc;
      if ((rc = tgmx_sgemm_nt_ep(h, ldh, ly.ch_w2, ly.ch_hidden, z_out, ldz, R, C, ly.ch_hidden, ly.ch_b2, 0, nullptr, 0, stream))) return rc;
      if ((rc = tgmx_dropout(z_out, ldz, R, C, &site[3], z_out, ldz, stream))) return rc;
      if ((rc = tgmx_add_cols(z_out, ldz, z1, ldz, R, C, 1, stream))) return rc;
    }
    z_in = z_out;
  }
  return TGMX_OK;
}

extern "C" int tgmx_mixer_token(const float* x, int64_t ldx, int64_t S, int32_t K, int32_t C, const float* tok_g, const float* tok_b,
                                const float* w1, const float* b1, int32_t Ht, const float* w2, const float* b2, const float* ch_g,
                                const float* ch_b, float eps, float* z1, float* y, int64_t ldo, tgmx_stream_t stream) {
  return mixer_token_run(false, x, ldx, S, K, C, tok_g, tok_b, w1, b1, Ht, w2, b2, ch_g, ch_b, eps, z1, y, ldo, stream);
}

extern "C" int tgmx_mixer_token_train(const float* x, int64_t ldx, int64_t S, int32_t K, int32_t C, const float* tok_g, const float* tok_b,
                                      const float* w1, const float* b1, int32_t Ht, const float* w2, const float* b2, const float* ch_g,
                                      const float* ch_b, float eps, float* z1, float* y, int64_t ldo, const tgmx_dropout_t* drop_hidden,
                                      const tgmx_dropout_t* drop_out, tgmx_stream_t stream) {
  return mixer_token_run(false, x, ldx, S, K, C, tok_g, tok_b, w1, b1, Ht, w2, b2, ch_g, ch_b, eps, z1, y, ldo, stream, drop_hidden, drop_out);
}

extern "C" int tgmx_tpnet_token_mix(const float* x, int64_t ldx, int64_t S, int32_t K, int32_t C, const float* tok_g, const float* tok_b,
                                    const float* w1, const float* b1, int32_t Ht, const float* w2, const float* b2, const float* ch_g,
                                    const float* ch_b, float eps, float* z1, float* y, int64_t ldo, tgmx_stream_t stream) {
  return mixer_token_run(true, x, ldx, S, K, C, tok_g, tok_b, w1, b1, Ht, w2, b2, ch_g, ch_b, eps, z1, y, ldo, stream);
}

extern "C" int tgmx_tpnet_token_mix_train(const float* x, int64_t ldx, int64_t S, int32_t K, int32_t C, const float* tok_g, const float* tok_b,
                                          const float* w1, const float* b1, int32_t Ht, const float* w2, const float* b2, const float* ch_g,
                                          const float* ch_b, float eps, float* z1, float* y, int64_t ldo, const tgmx_dropout_t* drop_hidden,
                                          const tgmx_dropout_t* drop_out, tgmx_stream_t stream) {
  return mixer_token_run(true, x, ldx, S, K, C, tok_g, tok_b, w1, b1, Ht, w2, b2, ch_g, ch_b, eps, z1, y, ldo, stream, drop_hidden, drop_out);
}

extern "C" int tgmx_mixer_tail(const float* z, int64_t ldz, int64_t S, int32_t K, int32_t C, const int32_t* nbr_nids, const float* node_x,
                               int64_t num_nodes, int32_t F, const int32_t* tg_nbr, const int32_t* tg_lo, const int32_t* tg_cnt,
                               const int32_t* seeds0, int64_t n0, const int32_t* seeds1, int64_t n1, const int32_t* seeds2, float* out,
                               int64_t ldo, tgmx_stream_t stream) {
  TGMX_REQUIRE(S >= 0 && K > 0 && C > 0 && F > 0 && num_nodes > 0 && ldz >= C && ldo >= C + F && n0 >= 0 && n1 >= 0 && n0 + n1 <= S,
               "mixer_tail: bad sizes S=%lld K=%d C=%d F=%d", (long long)S, K, C, F);
  if (S == 0) return TGMX_OK;
  TGMX_REQUIRE(z && nbr_nids && node_x && tg_lo && tg_cnt && out && (n0 == 0 || seeds0) && (n1 == 0 || seeds1) && (n0 + n1 == S || seeds2),
               "mixer_tail: null pointer");
  hipLaunchKernelGGL(mixer_tail_kernel, dim3((unsigned)S), dim3(kTailWaves * kWave), 0, (hipStream_t)stream, z, (long long)ldz, K, C, nbr_nids, node_x, F,
                     tg_nbr, tg_lo, tg_cnt, seeds0, (long long)n0, seeds1, (long long)n1, seeds2, out, (long long)ldo);
  TGMX_CHECK_LAUNCH("mixer_tail");
  return TGMX_OK;
}

// save_z / save_z1 (training, both or neither): layer l reads its input from save_z + l R ldz and leaves its token block's output in
// save_z1 + l R ldz -- the same launches in the same order as the inference call, writing elsewhere; drop: the sites' common descriptor
// (stream = the call's first stream; site s of layer l draws from stream + 4 l + s), NULL = off.
static int graphmixer_forward_run(const tgmx_graphmixer_fwd_t* a, float* save_z, float* save_z1, const tgmx_dropout_t* drop, tgmx_stream_t stream) {
  TGMX_REQUIRE(a && a->num_layers >= 0 && a->num_layers <= TGMX_MIXER_MAX_LAYERS, "graphmixer_forward: bad argument block");
  TGMX_REQUIRE(a->ldx0 % 4 == 0 && a->ldz % 4 == 0 && a->ldh % 4 == 0 && a->ldcat % 4 == 0, "graphmixer_forward: leading dimensions must be multiples of 4");
  TGMX_REQUIRE(a->n_seeds[0] + a->n_seeds[1] + a->n_seeds[2] == a->S, "graphmixer_forward: seed groups do not add up to S");
  const long long S = a->S, R = S * a->K;
  if (S == 0) return TGMX_OK;
  const int D = a->D, T = a->T, L = a->num_layers;
  const bool save = save_z != nullptr;
  const bool dropping = drop && drop->p > 0.f;
  TGMX_REQUIRE(save || !dropping, "graphmixer_forward: dropout is the training form's");
  int rc;
  if ((rc = tgmx_mixer_prologue(a->nbr_edge_x, a->seed_t, a->nbr_t, S, a->K, D, a->tw, a->tb, T, a->x0, a->ldx0, stream))) return rc;
  float* z_in = save && L > 0 ? save_z : a->z;
  if ((rc = tgmx_sgemm_nt_ep(a->x0, a->ldx0, a->proj_w, D + T, z_in, a->ldz, R, D, D + T, a->proj_b, 0, nullptr, 0, stream))) return rc;
  if (!save) {
    if ((rc = mixer_layers_run(false, a->layers, L, S, a->K, D, a->eps, a->z, a->z1, a->y, a->ldz, a->h, a->ldh, stream))) return rc;
  } else {
    if ((rc = mixer_layers_run_train(false, a->layers, L, S, a->K, D, a->eps, save_z, save_z1, a->z, a->y, a->ldz, a->h, a->ldh, drop, stream))) return rc;
  }
  if ((rc = tgmx_mixer_tail(a->z, a->ldz, S, a->K, D, a->nbr_nids, a->node_x, a->num_nodes, a->F, a->tg_nbr, a->tg_lo, a->tg_cnt, a->seeds[0],
                            a->n_seeds[0], a->seeds[1], a->n_seeds[1], a->seeds[2], a->cat, a->ldcat, stream)))
    return rc;
  return tgmx_sgemm_nt_ep(a->cat, a->ldcat, a->out_w, D + a->F, a->out, a->E, S, a->E, D + a->F, a->out_b, 0, nullptr, 0, stream);
}

extern "C" int tgmx_graphmixer_forward(const tgmx_graphmixer_fwd_t* a, tgmx_stream_t stream) {
  return graphmixer_forward_run(a, nullptr, nullptr, nullptr, stream);
}

extern "C" int tgmx_graphmixer_forward_train(const tgmx_graphmixer_fwd_t* a, float* save_z, float* save_z1, const tgmx_dropout_t* drop,
                                             tgmx_stream_t stream) {
  TGMX_REQUIRE(a && (a->num_layers == 0 || a->S == 0 || (save_z && save_z1)), "graphmixer_forward_train: the saving buffers are missing");
  static float none;  // (num_layers == 0: nothing is saved; the pointer only marks the training form)
  return graphmixer_forward_run(a, save_z ? save_z : &none, save_z1, drop, stream);
}
