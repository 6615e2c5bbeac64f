// The decoders (the reference's tgm/nn/decoder/{link,node,graph}proppred.py and tgm/nn/modules/aggregation.py) for gfx950: an MLP head over
// merged pairs of embedding rows, over rows, or over one pooled row.
//
// Two forms of the pair head.  PAIR: C = act(A1[ia] Wa^T + A2[ib] Wb^T + bias), the rows gathered through the indices into LDS, no [R, 2D]
// concatenation (ConcatMerge: Wa | Wb are the column halves of the first Linear; LearnableSumMerge: lin_src / lin_dst, act none).  TABLE:
// when both operands are rows of ONE table z [N', D], P = z [Wa ; Wb]^T + [bias | 0] is one GEMM over the table (tgmx_sgemm_nt) and the
// per-pair work is h = act(P[ia, :H] + P[ib, H:]) (tgmx_decoder_score), fused with the last Linear when that follows directly and is at
// most 16 wide.  Every sum has one fixed order (the K loop runs through the first operand, then the second, ascending; the row dots fold
// in a fixed butterfly; the pooling adds rows in ascending order, chunk by chunk): two runs give the same bits.  An index outside its
// table is never dereferenced: the pair's outputs are NaN and *bad counts it.
#include <math.h>

#include "common.h"

namespace tgmx {

using dec_f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kDecTM = 32, kDecTN = 64, kDecTK = 64;  // the pair GEMM's block: 32 rows x 64 columns, K staged 64 at a time
constexpr int kDecLd = kDecTK + 4;                    // LDS row pitch: the 16 x 4 operand reads of one MFMA land in 64 distinct banks
constexpr int kDecThreads = 256;
constexpr int kDecMaxTail = 16;    // widest last layer the row-dot kernels take
constexpr int kDecMaxH = 512;      // widest half row the score kernel keeps in LDS
constexpr int kDecChunk = 256;     // candidates (or flat pairs) per workgroup of the score / tail kernels
constexpr int kPoolRows = 128;     // rows per workgroup of the pooling's first stage

// ---- the pair form ------------------------------------------------------------------------------------------------------------------------
// v_mfma_f32_16x16x4_f32: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; D: col = l & 15, row = 4 (l >> 4) + reg.
// A wave owns 16 columns and both 16-row halves of the block (two accumulators sharing the weight operand).
__global__ __launch_bounds__(kDecThreads) void decoder_pair_gemm_kernel(const float* __restrict__ A1, long long lda1, long long n1,
                                                                        const int32_t* __restrict__ ia, const float* __restrict__ A2, long long lda2,
                                                                        long long n2, const int32_t* __restrict__ ib, const float* __restrict__ Wa,
                                                                        long long ldwa, int K1, const float* __restrict__ Wb, long long ldwb, int K2,
                                                                        const float* __restrict__ bias, int relu, float* __restrict__ C, long long ldc,
                                                                        long long R, int N, int* __restrict__ bad) {
  __shared__ float As[kDecTM * kDecLd];
  __shared__ float Ws[kDecTN * kDecLd];
  __shared__ long long s_row[2][kDecTM];  // the operand row behind each block row; -1: nothing to read (zeros), -2: index out of range
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long r0 = (long long)blockIdx.x * kDecTM;
  const int n0 = blockIdx.y * kDecTN;
  if (tid < 2 * kDecTM) {
    const int op = tid / kDecTM, i = tid % kDecTM;
    const long long r = r0 + i;
    long long src = -1;
    if (r < R && (op == 0 || A2)) {
      const int32_t* ix = op ? ib : ia;
      const long long v = ix ? (long long)ix[r] : r, nn = op ? n2 : n1;
      src = (v >= 0 && v < nn) ? v : -2;
      if (src == -2 && blockIdx.y == 0 && bad) atomicAdd(bad, 1);
    }
    s_row[op][i] = src;
  }
  __syncthreads();
  dec_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int op = 0; op < 2; ++op) {
    const float* A = op ? A2 : A1;
    if (!A) continue;
    const float* W = op ? Wb : Wa;
    const long long lda = op ? lda2 : lda1, ldw = op ? ldwb : ldwa;
    const int K = op ? K2 : K1;
    for (int k0 = 0; k0 < K; k0 += kDecTK) {
#pragma unroll
      for (int i = 0; i < kDecTM * kDecTK / kDecThreads; ++i) {
        const int e = tid + kDecThreads * i, row = e / kDecTK, k = e % kDecTK;
        const long long src = s_row[op][row];
        As[row * kDecLd + k] = (src >= 0 && k0 + k < K) ? A[src * lda + k0 + k] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < kDecTN * kDecTK / kDecThreads; ++i) {
        const int e = tid + kDecThreads * i, col = e / kDecTK, k = e % kDecTK;
        Ws[col * kDecLd + k] = (n0 + col < N && k0 + k < K) ? W[(long long)(n0 + col) * ldw + k0 + k] : 0.f;
      }
      __syncthreads();
      // Four accumulators per 16-row half take the chunk's 4-wide k-steps in turn (chains of at most 4 MFMAs = 16 products), fold as
      // (p0 + p1) + (p2 + p3), and the chunks add up in ascending order: short chains keep the rounding error near a blocked host sum's,
      // and four independent MFMAs cover the instruction's latency.  The staged tile is zero past K, so whole 16-wide steps are safe.
      const int kmax = min(kDecTK, (K - k0 + 15) & ~15);
      const float* ap = As + (lane & 15) * kDecLd + (lane >> 4);
      const float* bp = Ws + (wave * 16 + (lane & 15)) * kDecLd + (lane >> 4);
      dec_f32x4 p[4], q[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) p[s4] = q[s4] = dec_f32x4{0.f, 0.f, 0.f, 0.f};
      for (int kk = 0; kk < kmax; kk += 16) {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          const float b = bp[kk + 4 * s4];
          p[s4] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[kk + 4 * s4], b, p[s4], 0, 0, 0);
          q[s4] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[16 * kDecLd + kk + 4 * s4], b, q[s4], 0, 0, 0);
        }
      }
      acc0 += (p[0] + p[1]) + (p[2] + p[3]);
      acc1 += (q[0] + q[1]) + (q[2] + q[3]);
      __syncthreads();
    }
  }
  const int col = n0 + wave * 16 + (lane & 15);
  if (col >= N) return;
  const float bv = bias ? bias[col] : 0.f;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = half * 16 + 4 * (lane >> 4) + reg;
      const long long r = r0 + i;
      if (r >= R) continue;
      float v = __fadd_rn(half ? acc1[reg] : acc0[reg], bv);
      if (relu) v = v < 0.f ? 0.f : v;
      if (s_row[0][i] == -2 || s_row[1][i] == -2) v = __builtin_nanf("");
      C[r * ldc + col] = v;
    }
  }
}

// ---- the table form's per-pair stage --------------------------------------------------------------------------------------------------------
// Groups of G lanes (G a power of two, 8 .. 64, the smallest that covers H) take one pair each: lane g reads columns g, g + G, ...; the row
// dots fold over the group by xor shuffles from G / 2 down.  QUERIES: workgroup (b, chunk) keeps query b's half row P[ia[b], :H] in LDS for
// all its candidates (candidate 0 is ib[b], candidate j > 0 is neg[.. + j - 1]); FLAT: pair r reads P[ia[r], :H] and P[ib[r], H:].
// O > 0: out[row, o] = sum_c h_c wl[o, c] + bl[o] (wl in LDS);  O == 0: out[row, :H] = h.
template <bool FLAT>
__global__ __launch_bounds__(kDecThreads) void decoder_score_kernel(const float* __restrict__ P, long long ldp, long long NP, int H,
                                                                    const void* __restrict__ ia, const void* __restrict__ ib,
                                                                    const void* __restrict__ neg, int is64, const int64_t* __restrict__ off, long long M,
                                                                    long long count, int relu, const float* __restrict__ wl,
                                                                    const float* __restrict__ bl, int O, float* __restrict__ out, long long ldo, int G,
                                                                    int chunk, int* __restrict__ bad) {
  extern __shared__ float dec_lds[];
  float* s_q = dec_lds;                    // [H] (QUERIES)
  float* s_w = dec_lds + (FLAT ? 0 : H);   // [O, H]
  const int tid = threadIdx.x, g = tid / G, gl = tid % G, ngroups = kDecThreads / G;
  long long j0, j1, out_base = 0, neg_base = 0, qa = 0;
  bool q_ok = true;
  if (FLAT) {
    j0 = (long long)blockIdx.x * chunk;
    j1 = min(count, j0 + chunk);
  } else {
    const long long b = blockIdx.x;
    const long long cnt = 1 + (off ? (long long)(off[b + 1] - off[b]) : M);
    neg_base = off ? (long long)off[b] : b * M;
    out_base = neg_base + b;
    j0 = (long long)blockIdx.y * chunk;
    j1 = min(cnt, j0 + chunk);
    if (j0 >= j1) return;
    qa = ld_idx(ia, is64, b);
    q_ok = qa >= 0 && qa < NP;
    for (int c = tid; c < H; c += kDecThreads) s_q[c] = q_ok ? P[qa * ldp + c] : 0.f;
  }
  for (int e = tid; e < O * H; e += kDecThreads) s_w[e] = wl[e];
  __syncthreads();
  for (long long jj = j0; jj < j1; jj += ngroups) {  // every thread runs every trip: the shuffles below are in uniform flow
    const long long j = jj + g;
    const bool active = j < j1;
    long long a = qa, c = 0;
    bool ok = active && q_ok;
    if (active) {
      if (FLAT) {
        a = ld_idx(ia, is64, j);
        c = ld_idx(ib, is64, j);
        ok = a >= 0 && a < NP;
      } else {
        c = j == 0 ? ld_idx(ib, is64, blockIdx.x) : ld_idx(neg, is64, neg_base + j - 1);
      }
      ok = ok && c >= 0 && c < NP;
    }
    const float* qp = FLAT ? P + (ok ? a : 0) * ldp : s_q;
    const float* pp = P + (ok ? c : 0) * ldp + H;
    const long long row = out_base + j;
    float acc[kDecMaxTail];
#pragma unroll
    for (int o = 0; o < kDecMaxTail; ++o) acc[o] = 0.f;
    for (int col = gl; col < H; col += G) {
      float h = 0.f;
      if (ok) {
        h = __fadd_rn(qp[col], pp[col]);
        if (relu) h = h < 0.f ? 0.f : h;
      }
      if (O == 0) {
        if (active) out[row * ldo + col] = ok ? h : __builtin_nanf("");
      } else {
#pragma unroll
        for (int o = 0; o < kDecMaxTail; ++o)
          if (o < O) acc[o] = __fmaf_rn(h, s_w[o * H + col], acc[o]);
      }
    }
    if (O > 0) {
#pragma unroll
      for (int o = 0; o < kDecMaxTail; ++o) {
        if (o < O) {
          float v = acc[o];
          for (int sft = G >> 1; sft > 0; sft >>= 1) v += __shfl_xor(v, sft);
          if (active && gl == 0) out[row * O + o] = ok ? __fadd_rn(v, bl ? bl[o] : 0.f) : __builtin_nanf("");
        }
      }
    }
    if (active && !ok && gl == 0 && bad) atomicAdd(bad, 1);
  }
}

// out[r, o] = sum_c x[r, c] W[o, c] + b[o], O <= 16: one group of G lanes per row, the fold of the score kernel
__global__ __launch_bounds__(kDecThreads) void decoder_tail_kernel(const float* __restrict__ x, long long ldx, long long R, int K,
                                                                   const float* __restrict__ W, const float* __restrict__ b, int O,
                                                                   float* __restrict__ out, int G, int chunk) {
  extern __shared__ float dec_lds[];  // [O, K]
  const int tid = threadIdx.x, g = tid / G, gl = tid % G, ngroups = kDecThreads / G;
  for (int e = tid; e < O * K; e += kDecThreads) dec_lds[e] = W[e];
  __syncthreads();
  const long long j0 = (long long)blockIdx.x * chunk, j1 = min(R, j0 + chunk);
  for (long long jj = j0; jj < j1; jj += ngroups) {
    const long long r = jj + g;
    const bool active = r < j1;
    const float* xp = x + (active ? r : 0) * ldx;
    float acc[kDecMaxTail];
#pragma unroll
    for (int o = 0; o < kDecMaxTail; ++o) acc[o] = 0.f;
    for (int col = gl; col < K; col += G) {
      const float h = active ? xp[col] : 0.f;
#pragma unroll
      for (int o = 0; o < kDecMaxTail; ++o)
        if (o < O) acc[o] = __fmaf_rn(h, dec_lds[o * K + col], acc[o]);
    }
#pragma unroll
    for (int o = 0; o < kDecMaxTail; ++o) {
      if (o < O) {
        float v = acc[o];
        for (int sft = G >> 1; sft > 0; sft >>= 1) v += __shfl_xor(v, sft);
        if (active && gl == 0) out[r * O + o] = __fadd_rn(v, b ? b[o] : 0.f);
      }
    }
  }
}

// ---- pooling ----------------------------------------------------------------------------------------------------------------------------------
// stage 1: workgroup i adds rows [128 i, 128 i + 128): wave w takes rows w, w + 4, ... into four accumulators in turn (chains of 8 rows),
// folded (s0 + s1) + (s2 + s3); the four waves' sums fold the same way.  Stage 2 (a thread per column) adds the chunks into four
// accumulators in turn, folds them the same way and divides by N for the mean.  One chunk: stage 1 writes the result.  Short chains keep
// the rounding error near a pairwise sum's; the order never depends on anything but N.
__global__ __launch_bounds__(kDecThreads) void decoder_pool_chunk_kernel(const float* __restrict__ x, long long ldx, long long N, int D,
                                                                         double* __restrict__ part, float* __restrict__ out, int mean) {
  extern __shared__ double pool_lds[];  // [4, D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * kPoolRows, r1 = min(N, r0 + kPoolRows);
  for (int c = lane; c < D; c += kWave) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long r = r0 + wave; r < r1; r += 16) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (r + 4 * u < r1) s[u] += (double)x[(r + 4 * u) * ldx + c];
    }
    pool_lds[wave * D + c] = (s[0] + s[1]) + (s[2] + s[3]);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += kDecThreads) {
    const double s = (pool_lds[c] + pool_lds[D + c]) + (pool_lds[2 * D + c] + pool_lds[3 * D + c]);
    if (gridDim.x == 1) out[c] = (float)(mean ? s / (double)N : s);
    else part[(long long)blockIdx.x * D + c] = s;
  }
}

__global__ __launch_bounds__(kDecThreads) void decoder_pool_join_kernel(const double* __restrict__ part, int chunks, long long N, int D,
                                                                        float* __restrict__ out, int mean) {
  for (int c = blockIdx.x * kDecThreads + threadIdx.x; c < D; c += gridDim.x * kDecThreads) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < chunks; i += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i + u < chunks) s[u] += part[(long long)(i + u) * D + c];
    }
    const double t = (s[0] + s[1]) + (s[2] + s[3]);
    out[c] = (float)(mean ? t / (double)N : t);
  }
}

// ---- one row through the Linear layers ------------------------------------------------------------------------------------------------------
// R = 1 (GraphPredictor's pooled row, a single pair): ONE workgroup runs every layer, the row staying in LDS.  Wave w takes outputs w, w + 4,
// ...; lanes stride the inputs, accumulate in double and fold by a fixed butterfly; the sum is rounded to float32 once.  A GEMM block would
// be one workgroup's worth of work per layer too, with a launch each.
struct RowMlp {
  tgmx_decoder_layer_t ly[TGMX_DECODER_MAX_LAYERS];
  int n;
};
__global__ __launch_bounds__(kDecThreads) void decoder_row_mlp_kernel(const float* __restrict__ x, RowMlp m, int width, float* __restrict__ out) {
  extern __shared__ float dec_lds[];  // [2, width]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = threadIdx.x; c < m.ly[0].in; c += kDecThreads) dec_lds[c] = x[c];
  __syncthreads();
  for (int l = 0; l < m.n; ++l) {
    const float* xin = dec_lds + (l & 1) * width;
    float* xout = dec_lds + ((l + 1) & 1) * width;
    const int in = m.ly[l].in, no = m.ly[l].out;
    const bool last = l == m.n - 1;
    for (int j = wave; j < no; j += kDecThreads / kWave) {
      const float* w = m.ly[l].w + (long long)j * in;
      double acc = 0.0;
      for (int k = lane; k < in; k += kWave) acc = fma((double)xin[k], (double)w[k], acc);
#pragma unroll
      for (int sft = kWave / 2; sft > 0; sft >>= 1) acc += __shfl_xor(acc, sft);
      if (lane == 0) {
        float v = (float)(acc + (m.ly[l].b ? (double)m.ly[l].b[j] : 0.0));
        if (last) out[j] = v;
        else xout[j] = v < 0.f ? 0.f : v;
      }
    }
    __syncthreads();
  }
}

constexpr int kRowMlpMaxWidth = 4096;  // two rows in LDS
static bool dec_row_mlp_fits(const tgmx_decoder_fwd_t* a) {
  for (int l = 0; l < a->num_layers; ++l)
    if (a->layers[l].in > kRowMlpMaxWidth || a->layers[l].out > kRowMlpMaxWidth) return false;
  return true;
}

// rows (pairs) per workgroup of the flat score / tail kernels: one trip of the workgroup's groups while that still leaves fewer than ~1024
// workgroups, up to kDecChunk beyond (a single workgroup walking 200 rows is latency-bound: 50 dependent trips)
static int dec_chunk(long long rows, int G) {
  const int ngroups = kDecThreads / G;
  long long c = (rows / 1024 + ngroups - 1) / ngroups * ngroups;
  if (c < ngroups) c = ngroups;
  return (int)(c > kDecChunk ? kDecChunk : c);
}

static int dec_group(int width) {
  int g = 8;
  while (g < kWave && g < width) g <<= 1;
  return g;
}

}  // namespace tgmx

using namespace tgmx;

extern "C" int tgmx_decoder_pair_gemm(const float* A1, int64_t lda1, int64_t n1, const int32_t* ia, const float* A2, int64_t lda2, int64_t n2,
                                      const int32_t* ib, const float* Wa, int64_t ldwa, int32_t K1, const float* Wb, int64_t ldwb, int32_t K2,
                                      const float* bias, int32_t act, float* C, int64_t ldc, int64_t R, int32_t N, int32_t* bad,
                                      tgmx_stream_t stream) {
  TGMX_REQUIRE(act == TGMX_DECODER_ACT_NONE || act == TGMX_DECODER_ACT_RELU, "decoder_pair_gemm: unknown activation %d", act);
  TGMX_REQUIRE(R >= 0 && R < (1ll << 31) * kDecTM && N > 0 && K1 > 0 && lda1 >= K1 && ldwa >= K1 && ldc >= N && n1 >= 0,
               "decoder_pair_gemm: bad sizes R=%lld N=%d K1=%d", (long long)R, N, K1);
  TGMX_REQUIRE(!A2 || (K2 > 0 && lda2 >= K2 && ldwb >= K2 && n2 >= 0), "decoder_pair_gemm: bad sizes of the second operand K2=%d", K2);
  if (R == 0) return TGMX_OK;
  TGMX_REQUIRE(A1 && Wa && C && (!A2 || Wb), "decoder_pair_gemm: null pointer");
  TGMX_REQUIRE((ia || n1 >= R) && (!A2 || ib || n2 >= R), "decoder_pair_gemm: an operand without indices needs R rows");
  const dim3 grid((unsigned)((R + kDecTM - 1) / kDecTM), (unsigned)((N + kDecTN - 1) / kDecTN));
  hipLaunchKernelGGL(decoder_pair_gemm_kernel, grid, dim3(kDecThreads), 0, (hipStream_t)stream, A1, (long long)lda1, (long long)n1, ia, A2,
                     (long long)lda2, (long long)n2, ib, Wa, (long long)ldwa, K1, Wb, (long long)ldwb, A2 ? K2 : 0, bias, act, C, (long long)ldc,
                     (long long)R, N, bad);
  TGMX_CHECK_LAUNCH("decoder_pair_gemm");
  return TGMX_OK;
}

extern "C" int tgmx_decoder_score(const float* P, int64_t ldp, int64_t NP, int32_t H, const void* ia, const void* ib, const void* neg, int32_t idx64,
                                  const int64_t* off, int64_t M, int64_t max_candidates, int64_t B, int32_t act, const float* w_last,
                                  const float* b_last, int32_t out_dim, float* out, int64_t ldo, int32_t* bad, tgmx_stream_t stream) {
  TGMX_REQUIRE(act == TGMX_DECODER_ACT_NONE || act == TGMX_DECODER_ACT_RELU, "decoder_score: unknown activation %d", act);
  if (H <= 0 || H > kDecMaxH || out_dim < 0 || out_dim > kDecMaxTail) {
    set_error("decoder_score: H=%d (at most %d) or out_dim=%d (at most %d) outside the kernel's envelope", H, kDecMaxH, out_dim, kDecMaxTail);
    return TGMX_E_UNSUPPORTED;
  }
  TGMX_REQUIRE(B >= 0 && B < (1ll << 31) && NP >= 0 && ldp >= 2 * (int64_t)H && M >= -1 && (out_dim > 0 || ldo >= H),
               "decoder_score: bad sizes B=%lld M=%lld", (long long)B, (long long)M);
  if (B == 0) return TGMX_OK;
  TGMX_REQUIRE(P && ia && ib && out && (out_dim == 0 || w_last), "decoder_score: null pointer");
  const int G = dec_group(H);
  hipStream_t st = (hipStream_t)stream;
  if (M < 0) {  // flat pairs
    const size_t lds = (size_t)out_dim * H * sizeof(float);
    const int chunk = dec_chunk(B, G);
    hipLaunchKernelGGL(decoder_score_kernel<true>, dim3((unsigned)((B + chunk - 1) / chunk)), dim3(kDecThreads), lds, st, P, (long long)ldp,
                       (long long)NP, H, ia, ib, nullptr, idx64, nullptr, 0ll, (long long)B, act, w_last, b_last, out_dim, out, (long long)ldo, G, chunk,
                       bad);
  } else {
    const int64_t most = 1 + (off ? max_candidates : M);
    TGMX_REQUIRE((off ? max_candidates >= 0 : true) && most < (1ll << 24) * kDecChunk && (most == 1 || neg), "decoder_score: bad candidate lists");
    const size_t lds = (size_t)(out_dim + 1) * H * sizeof(float);
    hipLaunchKernelGGL(decoder_score_kernel<false>, dim3((unsigned)B, (unsigned)((most + kDecChunk - 1) / kDecChunk)), dim3(kDecThreads), lds, st, P,
                       (long long)ldp, (long long)NP, H, ia, ib, neg, idx64, off, (long long)M, (long long)B, act, w_last, b_last, out_dim, out,
                       (long long)ldo, G, kDecChunk, bad);
  }
  TGMX_CHECK_LAUNCH("decoder_score");
  return TGMX_OK;
}

extern "C" int tgmx_decoder_tail(const float* x, int64_t ldx, int64_t R, int32_t K, const float* W, const float* b, int32_t out_dim, float* out,
                                 tgmx_stream_t stream) {
  if (out_dim <= 0 || out_dim > kDecMaxTail || K <= 0 || (int64_t)out_dim * K * sizeof(float) > 48 * 1024) {
    set_error("decoder_tail: out_dim=%d (at most %d) K=%d outside the kernel's envelope", out_dim, kDecMaxTail, K);
    return TGMX_E_UNSUPPORTED;
  }
  TGMX_REQUIRE(R >= 0 && R < (1ll << 31) * kDecChunk && ldx >= K, "decoder_tail: bad sizes R=%lld", (long long)R);
  if (R == 0) return TGMX_OK;
  TGMX_REQUIRE(x && W && out, "decoder_tail: null pointer");
  const int G = dec_group(K), chunk = dec_chunk(R, G);
  hipLaunchKernelGGL(decoder_tail_kernel, dim3((unsigned)((R + chunk - 1) / chunk)), dim3(kDecThreads), (size_t)out_dim * K * sizeof(float),
                     (hipStream_t)stream, x, (long long)ldx, (long long)R, K, W, b, out_dim, out, G, chunk);
  TGMX_CHECK_LAUNCH("decoder_tail");
  return TGMX_OK;
}

extern "C" size_t tgmx_pool_rows_scratch_floats(int64_t N, int32_t D) {
  if (N <= kPoolRows || D <= 0) return 0;
  return 2 * (size_t)((N + kPoolRows - 1) / kPoolRows) * (size_t)D;  // (doubles)
}

extern "C" int tgmx_pool_rows(const float* x, int64_t ldx, int64_t N, int32_t D, int32_t mean, float* scratch, size_t scratch_floats, float* out,
                              tgmx_stream_t stream) {
  if (D <= 0 || D > 1536) {  // four partial rows of doubles in LDS
    set_error("pool_rows: D=%d outside the kernel's envelope", D);
    return TGMX_E_UNSUPPORTED;
  }
  TGMX_REQUIRE(N > 0 && N < (1ll << 31) * kPoolRows && ldx >= D && x && out, "pool_rows: bad sizes N=%lld or null pointer", (long long)N);
  const int64_t chunks = (N + kPoolRows - 1) / kPoolRows;
  TGMX_REQUIRE(chunks == 1 || (scratch && scratch_floats >= 2 * (size_t)chunks * D && ((uintptr_t)scratch & 7) == 0), "pool_rows: scratch too small or misaligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(decoder_pool_chunk_kernel, dim3((unsigned)chunks), dim3(kDecThreads), (size_t)4 * D * sizeof(double), st, x, (long long)ldx,
                     (long long)N, D, reinterpret_cast<double*>(scratch), out, mean ? 1 : 0);
  TGMX_CHECK_LAUNCH("pool_rows(chunks)");
  if (chunks > 1) {
    hipLaunchKernelGGL(decoder_pool_join_kernel, dim3((unsigned)((D + kDecThreads - 1) / kDecThreads)), dim3(kDecThreads), 0, st, reinterpret_cast<const double*>(scratch), (int)chunks,
                       (long long)N, D, out, mean ? 1 : 0);
    TGMX_CHECK_LAUNCH("pool_rows(join)");
  }
  return TGMX_OK;
}

extern "C" int tgmx_decoder_row_mlp(const float* x, const tgmx_decoder_layer_t* layers, int32_t num_layers, float* out, tgmx_stream_t stream) {
  TGMX_REQUIRE(x && layers && out && num_layers >= 1 && num_layers <= TGMX_DECODER_MAX_LAYERS, "decoder_row_mlp: null pointer or %d layers", num_layers);
  RowMlp m;
  m.n = num_layers;
  int width = 0;
  for (int l = 0; l < num_layers; ++l) {
    TGMX_REQUIRE(layers[l].w && layers[l].in > 0 && layers[l].out > 0 && (l == 0 || layers[l].in == layers[l - 1].out), "decoder_row_mlp: layer %d is malformed", l);
    m.ly[l] = layers[l];
    width = max(width, max(layers[l].in, layers[l].out));
  }
  if (width > kRowMlpMaxWidth) {
    set_error("decoder_row_mlp: width %d (at most %d) outside the kernel's envelope", width, kRowMlpMaxWidth);
    return TGMX_E_UNSUPPORTED;
  }
  hipLaunchKernelGGL(decoder_row_mlp_kernel, dim3(1), dim3(kDecThreads), (size_t)2 * width * sizeof(float), (hipStream_t)stream, x, m, width, out);
  TGMX_CHECK_LAUNCH("decoder_row_mlp");
  return TGMX_OK;
}

// the Linear layers after the merge stage: x [R, layers[0].in] -> out [R, layers[L - 1].out]; relu between, none after the last
static int decoder_layers(const tgmx_decoder_fwd_t* a, const float* x, int64_t ldx, int64_t R, int first, tgmx_stream_t stream) {
  int rc, flip = 0;
  if (R == 1 && dec_row_mlp_fits(a)) return tgmx_decoder_row_mlp(x, a->layers, a->num_layers, a->out, stream);
  for (int l = first; l < a->num_layers; ++l) {
    const tgmx_decoder_layer_t& ly = a->layers[l];
    const bool last = l == a->num_layers - 1;
    if (last && ly.out <= kDecMaxTail && (int64_t)ly.out * ly.in * sizeof(float) <= 48 * 1024) return tgmx_decoder_tail(x, ldx, R, ly.in, ly.w, ly.b, ly.out, a->out, stream);
    float* y = last ? a->out : a->h[flip];
    TGMX_REQUIRE(y, "decoder_forward: no buffer for layer %d's output", l);
    if ((rc = tgmx_sgemm_nt(x, ldx, ly.w, ly.in, y, ly.out, R, ly.out, ly.in, ly.b, last ? 0 : 1, 1, 0, 0, 0, stream))) return rc;
    x = y;
    ldx = ly.out;
    flip ^= 1;
  }
  return TGMX_OK;
}

extern "C" int tgmx_decoder_forward(const tgmx_decoder_fwd_t* a, tgmx_stream_t stream) {
  TGMX_REQUIRE(a, "decoder_forward: null argument block");
  TGMX_REQUIRE(a->num_layers >= 1 && a->num_layers <= TGMX_DECODER_MAX_LAYERS && a->out, "decoder_forward: %d layers", a->num_layers);
  for (int l = 0; l < a->num_layers; ++l) {
    TGMX_REQUIRE(a->layers[l].w && a->layers[l].in > 0 && a->layers[l].out > 0 && (l == 0 || a->layers[l].in == a->layers[l - 1].out),
                 "decoder_forward: layer %d is malformed", l);
  }
  int rc;
  const int D = a->D, H = a->H;
  switch (a->form) {
    case TGMX_DECODER_ROWS: {
      const float* x = a->a1;
      int64_t R = a->R, ldx = a->lda1;
      TGMX_REQUIRE(x && ldx >= D && D == a->layers[0].in, "decoder_forward(rows): bad operand");
      if (a->pool != TGMX_DECODER_POOL_NONE) {
        TGMX_REQUIRE(a->pooled, "decoder_forward(rows): no buffer for the pooled row");
        if ((rc = tgmx_pool_rows(x, ldx, a->n1, D, a->pool == TGMX_DECODER_POOL_MEAN, a->pool_ws, a->pool_ws_floats, a->pooled, stream))) return rc;
        x = a->pooled;
        ldx = D;
        R = 1;
      }
      return decoder_layers(a, x, ldx, R, 0, stream);
    }
    case TGMX_DECODER_PAIR: {
      TGMX_REQUIRE(a->h[1] && H > 0 && H == a->layers[0].in, "decoder_forward(pair): the merge stage needs h[1] and H = the first layer's width");
      if ((rc = tgmx_decoder_pair_gemm(a->a1, a->lda1, a->n1, static_cast<const int32_t*>(a->ia), a->a2, a->lda2, a->n2,
                                       static_cast<const int32_t*>(a->ib), a->wa, a->ldwa, D, a->wb, a->ldwb, D, a->mbias, a->merge_act, a->h[1], H,
                                       a->R, H, a->bad, stream)))
        return rc;
      // (the layers flip from h[0]: the merge's output in h[1] is the first one's input)
      return decoder_layers(a, a->h[1], H, a->R, 0, stream);
    }
    case TGMX_DECODER_TABLE: {
      TGMX_REQUIRE(a->P && a->a1 && a->wa && H > 0 && H == a->layers[0].in && a->lda1 >= D, "decoder_forward(table): bad operand");
      if (a->n1 == 0 || a->B == 0) return TGMX_OK;
      if ((rc = tgmx_sgemm_nt(a->a1, a->lda1, a->wa, a->ldwa, a->P, 2 * (int64_t)H, a->n1, 2 * H, D, a->mbias, 0, 1, 0, 0, 0, stream))) return rc;
      const tgmx_decoder_layer_t& ly = a->layers[0];
      const bool fuse = a->num_layers == 1 && ly.out <= kDecMaxTail && a->merge_act == TGMX_DECODER_ACT_RELU;
      if (fuse)
        return tgmx_decoder_score(a->P, 2 * (int64_t)H, a->n1, H, a->ia, a->ib, a->neg, a->idx64, a->off, a->M, a->max_candidates, a->B, a->merge_act,
                                  ly.w, ly.b, ly.out, a->out, 0, a->bad, stream);
      TGMX_REQUIRE(a->h[1], "decoder_forward(table): the unfused head needs h[1]");
      if ((rc = tgmx_decoder_score(a->P, 2 * (int64_t)H, a->n1, H, a->ia, a->ib, a->neg, a->idx64, a->off, a->M, a->max_candidates, a->B, a->merge_act,
                                   nullptr, nullptr, 0, a->h[1], H, a->bad, stream)))
        return rc;
      return decoder_layers(a, a->h[1], H, a->R, 0, stream);
    }
    default:
      set_error("decoder_forward: unknown form %d", a->form);
      return TGMX_E_INVALID;
  }
}
