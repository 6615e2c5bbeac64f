// The dense library (fp32) for gfx950 that every model of the package calls into: tgmx_sgemm_nt, tgmx_sgemm_nt_ep and
// tgmx_internal_sgemm_nt_pair (C = act(A B^T + bias) (+ res) on the exact-fp32 MFMA: four kernels, one routing rule, gemm_route), and the
// row primitives tgmx_gather_rows, tgmx_time2vec, tgmx_dropout, tgmx_pack2d, tgmx_layernorm_rows.  load_kn and floatx16: gemm.h.
#include "common.h"
#include "gemm.h"

#include <type_traits>

namespace tgmx {

// ---------------------------------------------------------------------------
// C[M,N] = act(A[M,K] * B[N,K]^T + bias[N]);  row-major, arbitrary leading dims,
// optional batch (grid.z) with element strides.  Exact-fp32 MFMA
// (v_mfma_f32_32x32x2_f32), operands loaded STRAIGHT INTO THE MFMA REGISTER LAYOUT:
// both A and B are K-contiguous, so lane (i = lane & 31, half = lane >> 5) loads the
// 8 consecutive k of "its" row -- A[m0+i][k0 + 8*half ..] and B[n0+i][k0 + 8*half ..]
// (two 16-byte loads each) -- and the kk-th MFMA of a 16-wide k step consumes
// k0+kk from the lower half-wave and k0+8+kk from the upper one.  No LDS, no
// barriers; a wave owns a 32 x 64 output tile (two accumulators), four waves stack
// along M.  The next step's operands are loaded before the current step's 16 MFMAs.
// ---------------------------------------------------------------------------
struct GemmArgs {
  const float* A;
  const float* B;
  float* C;
  const float* bias;
  long long lda, ldb, ldc, sA, sB, sC;
  long long M;
  int N, K, relu;  // epilogue activation: 0 none, 1 ReLU, 2 exact-erf GELU (tgmx_sgemm_nt_ep)
  const float* res = nullptr;  // tgmx_sgemm_nt_ep: [M, N] (leading dimension ldr) added after the activation
  long long ldr = 0;
};

// bias, activation, residual of one output element (the ReLU path is the arithmetic tgmx_sgemm_nt always had)
__device__ __forceinline__ float gemm_act_res(const GemmArgs& g, float v, long long row, int col, unsigned bz) {
  if (g.relu == 1) v = v > 0.f ? v : 0.f;
  else if (g.relu == 2) v = 0.5f * v * (1.f + erff(v * 0.70710678118654752f));  // torch.nn.GELU(approximate='none')
  if (g.res) v += g.res[(long long)bz * g.sC + row * g.ldr + col];
  return v;
}

// One k-step covers 2 * kGemmK columns of K: lanes 0-31 hold the first kGemmK of their row, lanes 32-63 the next
// kGemmK (any pairing of k with the two k-slots of the 32x32x2 MFMA is valid as long as A and B agree).
// kGemmK = 8 measured best on this path's skinny GEMMs (16 / 32 cost occupancy: 216+ VGPRs, one wave per SIMD).
//
// C[M, N] = A[M, K] . B[N, K]^T (+ bias, relu), both operands K-contiguous and loaded straight into the MFMA
// register layout (no LDS staging).  SPLIT = false: the 4 waves of a block own 4 row tiles (128 rows).
// SPLIT = true (few tiles): the 4 waves share ONE 32 x 64 tile, wave w takes k-steps w, w + 4, ... and the
// partial tiles meet in LDS (fixed summation order: deterministic).
// EXT: the K-split reduction's 32 KB live in LDS the caller provides (a kernel that also instantiates the LDS-staged body: one buffer for both)
template <bool AV, bool BV, bool SPLIT, int kGemmK, bool EXT = false>
__device__ __forceinline__ void sgemm_nt_body(const GemmArgs& g, const unsigned bx, const unsigned by, const unsigned bz, float* ext = nullptr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, half = lane >> 5;
  const long long m0 = SPLIT ? (long long)bx * 32 : (long long)bx * 128 + wave * 32;
  if (!SPLIT && m0 >= g.M) return;  // whole wave out of range (no block-level sync on this path)
  const int n0 = by * 64;
  const float* __restrict__ A = g.A + (long long)bz * g.sA;
  const float* __restrict__ B = g.B + (long long)bz * g.sB;
  float* __restrict__ C = g.C + (long long)bz * g.sC;
  // rows / columns past the edge are clamped for the loads; their results are never stored
  const long long ra = m0 + i < g.M ? m0 + i : g.M - 1;
  const int c0 = n0 + i < g.N ? n0 + i : g.N - 1;
  const int c1 = n0 + 32 + i < g.N ? n0 + 32 + i : g.N - 1;
  const float* __restrict__ pa = A + ra * g.lda;
  const float* __restrict__ pb0 = B + (long long)c0 * g.ldb;
  const float* __restrict__ pb1 = B + (long long)c1 * g.ldb;

  floatx16 acc0 = {0}, acc1 = {0};
  float a[kGemmK], b0[kGemmK], b1[kGemmK], an[kGemmK], b0n[kGemmK], b1n[kGemmK];
  constexpr int kStep = 2 * kGemmK;
  const int stride = SPLIT ? 4 * kStep : kStep;
  int k0 = SPLIT ? wave * kStep : 0;
  if (k0 < g.K) {
    load_kn<AV, kGemmK>(pa, k0 + half * kGemmK, g.K, a);
    load_kn<BV, kGemmK>(pb0, k0 + half * kGemmK, g.K, b0);
    load_kn<BV, kGemmK>(pb1, k0 + half * kGemmK, g.K, b1);
  }
  for (; k0 < g.K; k0 += stride) {
    const bool more = k0 + stride < g.K;
    if (more) {
      const int kb = k0 + stride + half * kGemmK;
      load_kn<AV, kGemmK>(pa, kb, g.K, an);
      load_kn<BV, kGemmK>(pb0, kb, g.K, b0n);
      load_kn<BV, kGemmK>(pb1, kb, g.K, b1n);
    }
#pragma unroll
    for (int kk = 0; kk < kGemmK; ++kk) {
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b0[kk], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b1[kk], acc1, 0, 0, 0);
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < kGemmK; ++u) {
        a[u] = an[u];
        b0[u] = b0n[u];
        b1[u] = b1n[u];
      }
    }
  }
  if (SPLIT) {
    float (*part)[32][kWave];  // [wave][acc register (0-15: acc0, 16-31: acc1)][lane]
    if constexpr (EXT) {
      part = reinterpret_cast<float (*)[32][kWave]>(ext);
    } else {
      __shared__ float part_own[4][32][kWave];
      part = part_own;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      part[wave][r][lane] = acc0[r];
      part[wave][16 + r][lane] = acc1[r];
    }
    __syncthreads();
    // wave w finishes registers 8w .. 8w+7 of every lane
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int rr = wave * 8 + q;
      float v = part[0][rr][lane] + part[1][rr][lane] + part[2][rr][lane] + part[3][rr][lane];
      const int r = rr & 15, t = rr >> 4;
      const long long row = m0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const int col = n0 + t * 32 + i;
      if (row < g.M && col < g.N) {
        if (g.bias) v += g.bias[(long long)bz * g.N + col];  // batch b adds row b of a [batch, N] bias
        C[row * g.ldc + col] = gemm_act_res(g, v, row, col, bz);
      }
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long row = m0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (row >= g.M) continue;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = n0 + t * 32 + i;
      if (col < g.N) {
        float v = t ? acc1[r] : acc0[r];
        if (g.bias) v += g.bias[(long long)bz * g.N + col];  // batch b adds row b of a [batch, N] bias
        C[row * g.ldc + col] = gemm_act_res(g, v, row, col, bz);
      }
    }
  }
}

template <bool AV, bool BV, bool SPLIT, int kGemmK>
__global__ __launch_bounds__(256) void sgemm_nt_kernel(const GemmArgs g) {
  sgemm_nt_body<AV, BV, SPLIT, kGemmK>(g, blockIdx.x, blockIdx.y, blockIdx.z);
}

// TWO independent GEMMs in one launch (the K-split kernel's body, unchanged: each problem's result is bit for bit what its own launch gives).
// Workgroups [0, tiles0) of the x dimension belong to problem 0, the rest to problem 1; the y / z extents are the larger of the two
// problems' (a workgroup outside its problem's extent returns at once).  For pairs that do not depend on each other and are each too
// small to fill the chip -- the GRU's gi / gh, TransformerConv's node projections / edge projection (cfg 3: four launches of ~14 us -> two).
struct GemmPairArgs {
  GemmArgs g[2];
  unsigned tiles0, ny[2], nz[2];
  int lds[2];  // (mixed pairs) the problem takes the LDS-staged body
};

__global__ __launch_bounds__(256) void sgemm_nt_pair_kernel(const GemmPairArgs p) {
  const unsigned which = blockIdx.x >= p.tiles0;
  if (blockIdx.y >= p.ny[which] || blockIdx.z >= p.nz[which]) return;
  if (which) sgemm_nt_body<true, true, true, 8>(p.g[1], blockIdx.x - p.tiles0, blockIdx.y, blockIdx.z);
  else sgemm_nt_body<true, true, true, 8>(p.g[0], blockIdx.x, blockIdx.y, blockIdx.z);
}

// The MANY-ROW variant (M >= 6144, see gemm_route): both operands STAGED THROUGH LDS in whole 128-byte lines.
// Why: the direct kernel above takes 32 bytes of every 128-byte line per lane and k-step straight from L2 into the
// MFMA layout; with 4-5 workgroups per CU in flight the lines do not survive in the 32 KB L1 until their other quarters are wanted, and the
// launch runs at 0.22-0.34 of the fp32-MFMA peak however it is tiled (12 600 x 172 x 172: 23 us for 4.8 us of MFMAs, ~4 us per layer of
// 256 workgroups).  Here a workgroup owns a 64 x 64 block; per 32-wide k-chunk its 256 threads fetch the block's 64 + 64 rows as 128-byte
// row segments (eight lanes x 16 bytes per row: every line whole, once), park them in registers while the current chunk's MFMAs run, and
// store them into the other LDS buffer (rows padded to 36 floats: conflict-free 16-byte reads).  Wave (wr, wc) multiplies rows
// [32 wr, 32 wr + 32) with columns [32 wc, 32 wc + 32): lane (i, half) reads k-set [16 half, 16 half + 16) of its A row and its B row (four
// 16-byte LDS reads each) for the chunk's 16 MFMAs -- the same pairing of k with the two k-slots as above.  One barrier per chunk.
// Summation order: chunk by chunk in ascending k, no cross-wave reduction (differs from the K-split kernel at rounding level).
constexpr int kLdsBM = 64, kLdsBN = 64, kLdsBK = 32, kLdsLd = kLdsBK + 4;
constexpr int kLdsFloats = 2 * (kLdsBM + kLdsBN) * kLdsLd;  // two buffers of (A block | B block): 36 864 bytes

// one 16-byte piece of a row's k-chunk: zeros past K (K need not be a multiple of 4; the padding of a padded row is not trusted)
// (VEC = false: rows that are not 16-byte aligned -- column-sliced views -- are read float by float: same values, same sums)
template <bool VEC>
__device__ __forceinline__ float4 lds_gemm_piece(const float* __restrict__ row, int k, int K) {
  if (VEC && k + 4 <= K) return *reinterpret_cast<const float4*>(row + k);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (k < K) v.x = row[k];
  if (k + 1 < K) v.y = row[k + 1];
  if (k + 2 < K) v.z = row[k + 2];
  if (k + 3 < K) v.w = row[k + 3];
  return v;
}

template <bool AV, bool BV>
__device__ __forceinline__ void sgemm_nt_lds_body(const GemmArgs& g, const unsigned bx, const unsigned by, const unsigned bz, float* __restrict__ smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 31, half = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const long long m0 = (long long)bx * kLdsBM;
  const int n0 = by * kLdsBN;
  const float* __restrict__ A = g.A + (long long)bz * g.sA;
  const float* __restrict__ B = g.B + (long long)bz * g.sB;
  float* __restrict__ C = g.C + (long long)bz * g.sC;
  // staging: thread t moves piece (t & 7) of rows (t >> 3) and (t >> 3) + 32 of the A block and of the B block (rows past the edge are
  // clamped: their products are never stored)
  const int sr = tid >> 3, sc = (tid & 7) * 4;
  const long long ra0 = m0 + sr < g.M ? m0 + sr : g.M - 1, ra1 = m0 + sr + 32 < g.M ? m0 + sr + 32 : g.M - 1;
  const int rb0 = n0 + sr < g.N ? n0 + sr : g.N - 1, rb1 = n0 + sr + 32 < g.N ? n0 + sr + 32 : g.N - 1;
  const float* __restrict__ pa0 = A + ra0 * g.lda;
  const float* __restrict__ pa1 = A + ra1 * g.lda;
  const float* __restrict__ pb0 = B + (long long)rb0 * g.ldb;
  const float* __restrict__ pb1 = B + (long long)rb1 * g.ldb;
  auto As = [&](int buf) { return smem + buf * (kLdsBM + kLdsBN) * kLdsLd; };
  auto Bs = [&](int buf) { return smem + buf * (kLdsBM + kLdsBN) * kLdsLd + kLdsBM * kLdsLd; };
  const int nchunks = (g.K + kLdsBK - 1) / kLdsBK;
  float4 v[4];  // the thread's four staged pieces: rows sr and sr + 32 of the A block and of the B block
  auto request = [&](int chunk) __attribute__((always_inline)) {
    const int k = chunk * kLdsBK + sc;
    v[0] = lds_gemm_piece<AV>(pa0, k, g.K); v[1] = lds_gemm_piece<AV>(pa1, k, g.K);
    v[2] = lds_gemm_piece<BV>(pb0, k, g.K); v[3] = lds_gemm_piece<BV>(pb1, k, g.K);
  };
  auto park = [&](int buf) __attribute__((always_inline)) {
    *reinterpret_cast<float4*>(As(buf) + sr * kLdsLd + sc) = v[0];
    *reinterpret_cast<float4*>(As(buf) + (sr + 32) * kLdsLd + sc) = v[1];
    *reinterpret_cast<float4*>(Bs(buf) + sr * kLdsLd + sc) = v[2];
    *reinterpret_cast<float4*>(Bs(buf) + (sr + 32) * kLdsLd + sc) = v[3];
  };
  request(0);
  park(0);
  __syncthreads();
  floatx16 acc = {0};
  for (int c = 0; c < nchunks; ++c) {
    const bool more = c + 1 < nchunks;
    if (more) request(c + 1);  // the next chunk's lines: in flight during this chunk's MFMAs
    const float4* __restrict__ ar = reinterpret_cast<const float4*>(As(c & 1) + (wr * 32 + i) * kLdsLd + half * 16);
    const float4* __restrict__ br = reinterpret_cast<const float4*>(Bs(c & 1) + (wc * 32 + i) * kLdsLd + half * 16);
    float4 a4[4], b4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { a4[u] = ar[u]; b4[u] = br[u]; }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u].x, b4[u].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u].y, b4[u].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u].z, b4[u].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u].w, b4[u].w, acc, 0, 0, 0);
    }
    if (more) {  // (the other buffer was last read in iteration c - 1, behind that iteration's barrier)
      park((c + 1) & 1);
      __syncthreads();
    }
  }
  const int col = n0 + wc * 32 + i;
  if (col < g.N) {
    const float bias = g.bias ? g.bias[(long long)bz * g.N + col] : 0.f;  // batch b adds row b of a [batch, N] bias
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long row = m0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (row < g.M) {
        float v = acc[r];
        if (g.bias) v += bias;
        C[row * g.ldc + col] = gemm_act_res(g, v, row, col, bz);
      }
    }
  }
}

template <bool AV, bool BV>
__global__ __launch_bounds__(256) void sgemm_nt_lds_kernel(const GemmArgs g) {
  __shared__ __attribute__((aligned(16))) float smem[kLdsFloats];
  sgemm_nt_lds_body<AV, BV>(g, blockIdx.x, blockIdx.y, blockIdx.z, smem);
}

// two independent problems in one launch of the kernel above (see sgemm_nt_pair_kernel)
__global__ __launch_bounds__(256) void sgemm_nt_lds_pair_kernel(const GemmPairArgs p) {
  __shared__ __attribute__((aligned(16))) float smem[kLdsFloats];
  const unsigned which = blockIdx.x >= p.tiles0;
  if (blockIdx.y >= p.ny[which] || blockIdx.z >= p.nz[which]) return;
  sgemm_nt_lds_body<true, true>(p.g[which], which ? blockIdx.x - p.tiles0 : blockIdx.x, blockIdx.y, blockIdx.z, smem);
}

// ... and a pair whose problems take DIFFERENT kernels alone (cfg 3's projections: ~5 k unique nodes beside ~13 k edges): each through
// its own body, unchanged, over one LDS buffer -- still one launch, and each result bit for bit what its own launch gives
__global__ __launch_bounds__(256) void sgemm_nt_mixed_pair_kernel(const GemmPairArgs p) {
  __shared__ __attribute__((aligned(16))) float smem[kLdsFloats];
  static_assert(kLdsFloats >= 4 * 32 * kWave, "the K-split reduction fits the staging buffer");
  const unsigned which = blockIdx.x >= p.tiles0;
  if (blockIdx.y >= p.ny[which] || blockIdx.z >= p.nz[which]) return;
  const unsigned bx = which ? blockIdx.x - p.tiles0 : blockIdx.x;
  if (p.lds[which]) sgemm_nt_lds_body<true, true>(p.g[which], bx, blockIdx.y, blockIdx.z, smem);
  else sgemm_nt_body<true, true, true, 8, true>(p.g[which], bx, blockIdx.y, blockIdx.z, smem);
}

// The FEW-ROW variant (M <= 2048: the 600-row layer of the headline forward, whose five GEMMs were 41 us of a 185 us forward at ~8 us
// each for 0.03-0.2 GFLOP).  Such a launch is one dependent chain -- launch, operand latency, MFMAs, reduction, store -- so the
// kernel is built to make that chain SHORT instead of wide: a workgroup owns one 32 x 32 output block, its 8 waves split K into
// contiguous slices of STEPS 16-wide steps, and a wave issues EVERY load of its slice before its first MFMA (<= 16 float4 per lane:
// one memory latency per launch, where sgemm_nt_kernel<SPLIT> pays one per k-step: 4-7 of them).  The 8 partial blocks meet in LDS
// in wave order (fixed: deterministic).  32-column blocks instead of 64 double the workgroups (114 for a 600 x 172 output).
template <bool AV, bool BV, int STEPS>
__global__ __launch_bounds__(512) void sgemm_nt_small_kernel(const GemmArgs g) {
  constexpr int kW = 8;
  __shared__ float part[kW][16][kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, half = lane >> 5;
  const long long m0 = (long long)blockIdx.x * 32;
  const int n0 = blockIdx.y * 32;
  const float* __restrict__ A = g.A + (long long)blockIdx.z * g.sA;
  const float* __restrict__ B = g.B + (long long)blockIdx.z * g.sB;
  float* __restrict__ C = g.C + (long long)blockIdx.z * g.sC;
  const long long ra = m0 + i < g.M ? m0 + i : g.M - 1;  // clamped for the loads; never stored
  const int cb = n0 + i < g.N ? n0 + i : g.N - 1;
  const float* __restrict__ pa = A + ra * g.lda;
  const float* __restrict__ pb = B + (long long)cb * g.ldb;
  const int kbeg = wave * STEPS * 16;
  float a[STEPS][8], b[STEPS][8];
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    const int k0 = kbeg + st * 16;
    if (k0 < g.K) {
      load_kn<AV, 8>(pa, k0 + half * 8, g.K, a[st]);
      load_kn<BV, 8>(pb, k0 + half * 8, g.K, b[st]);
    }
  }
  floatx16 acc = {0};
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    if (kbeg + st * 16 < g.K) {
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[st][kk], b[st][kk], acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) part[wave][r][lane] = acc[r];
  __syncthreads();
  // wave w finishes accumulator registers 2w and 2w + 1 of every lane
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int r = wave * 2 + q;
    float v = part[0][r][lane];
#pragma unroll
    for (int w = 1; w < kW; ++w) v += part[w][r][lane];
    const long long row = m0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    const int col = n0 + i;
    if (row < g.M && col < g.N) {
      if (g.bias) v += g.bias[(long long)blockIdx.z * g.N + col];
      C[row * g.ldc + col] = gemm_act_res(g, v, row, col, blockIdx.z);
    }
  }
}

// ---------------------------------------------------------------------------
// out[i, :] = table[idx[i] (negative wraps, like Python indexing), :]
// (tgat.py:128-130: pad id -1 reads the LAST row of node_x)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ table, long long rows, int dim,
                                                          const int32_t* __restrict__ idx, long long n,
                                                          float* out, long long ldo) {
  const long long total = n * dim;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
    const long long i = e / dim;
    const int c = (int)(e - i * dim);
    long long r = idx[i];
    if (r < 0) r += rows;
    out[i * ldo + c] = table[r * dim + c];
  }
}

// out[i, t] = cos(fma(float(x[i]), w[t], b[t]))   (Time2Vec.forward, time_encoding.py:22-24)
template <typename TI>
__global__ __launch_bounds__(256) void time2vec_kernel(const TI* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ b, int T, long long n,
                                                       float* __restrict__ out) {
  const long long total = n * T;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
    const long long i = e / T;
    const int t = (int)(e - i * T);
    out[e] = cos_t2v(__fmaf_rn((float)x[i], w[t], b[t]));
  }
}

// LayerNorm over rows (DyGFormer's token rows): one wave per row, biased variance; columns [d, ldy) of y are left alone
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const float* __restrict__ x, long long ldx, long long R, int d,
                                                            const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                            float* __restrict__ y, long long ldy) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long r = (long long)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
  if (r >= R) return;
  const float* __restrict__ row = x + r * ldx;
  float sum = 0.f;
  for (int c = lane; c < d; c += kWave) sum += row[c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  const float mean = sum / (float)d;
  float var = 0.f;
  for (int c = lane; c < d; c += kWave) {
    const float t = row[c] - mean;
    var = __fmaf_rn(t, t, var);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) var += __shfl_xor(var, o);
  const float rstd = 1.f / sqrtf(var / (float)d + eps);
  float* __restrict__ yo = y + r * ldy;
  for (int c = lane; c < d; c += kWave) yo[c] = (row[c] - mean) * rstd * g[c] + b[c];
}

__global__ __launch_bounds__(256) void dropout_kernel(const float* x, long long ldx, long long R, int C, DropoutArgs d, long long row0,
                                                      float* out, long long ldo) {
  const long long total = R * C;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long r = e / C;
    const int c = (int)(e - r * C);
    out[r * ldo + c] = x[r * ldx + c] * dropout_scale(d, (unsigned long long)(row0 + r) * C + c);
  }
}

}  // namespace tgmx

using namespace tgmx;

// Which problems take the LDS-staged kernel: M >= 6144 rows.  A function of M ALONE, like the few-row kernel's M <= 2048: the levels of a
// hop tree that share a layer's weights run as one row batch in one composition and level by level in another (12 600 = 600 + 12 000
// rows: tests/test_tgat_backward_gpu.py compares the two bit for bit), and a threshold on the number of 64 x 64 blocks -- which fits the
// measurements a little better (8 118 x 172 x 172, 381 blocks: 13.4 us direct / 14.0 staged; 8 118 x 200 x 116, 508 blocks: 14.0 / 11.2)
// -- put 12 000 x 51 x 273 x 2 heads and 12 600 x 51 x 273 x 2 heads on different sides.  Below ~6 k rows a launch is at most 1.5 rounds of
// blocks per CU and the K-split kernel's four short chains per 32 x 64 tile finish sooner (4 100 x 172 x 172: 8.3 / 10.4 us).
constexpr long long kGemmLdsMinRows = 6144;

// THE routing rule: which kernel a problem takes, alone (sgemm_nt_run) or as half of a pair (tgmx_internal_sgemm_nt_pair).  A function
// of M, K and the two A/B knobs only (TGMX_GEMM_SMALL=0: no few-row kernel, TGMX_GEMM_LDS=0: no LDS-staged kernel), never of N, the
// batch or the operands' alignment (alignment picks the AV / BV instantiation of the routed kernel, see gemm_by_vec):
//   K <= 16          any M                direct    sgemm_nt_kernel<SPLIT = false>: one k-step, nothing to split
//   16 < K <= 512    M <= 2048            few-row   sgemm_nt_small_kernel             (TGMX_GEMM_SMALL=0: K-split)
//   K > 16           M >= 6144            LDS       sgemm_nt_lds_kernel               (TGMX_GEMM_LDS=0: K-split)
//   K > 16           every other M        K-split   sgemm_nt_kernel<SPLIT = true>     (2048 < M < 6144; M <= 2048 with K > 512)
// K-splitting across the 4 waves of a block (4x the waves, each with a quarter of the dependent MFMA chain) wins whenever there is more
// than one 16-wide k-step to hand out; measured on every GEMM shape of the TGAT path (600 .. 12 600 rows, K = 102 .. 448: 1.1x .. 2.9x)
// and neutral at 4096^3.  The few-row kernel was tried up to 64 k rows on the TGN pipeline's GEMMs: no gain past ~2 k.
enum class GemmRoute { kFewRow, kLds, kKSplit, kDirect };
static GemmRoute gemm_route(long long M, int K) {
  static const auto knob = [](const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); };
  static const bool small_knob = knob("TGMX_GEMM_SMALL"), lds_knob = knob("TGMX_GEMM_LDS");
  if (K <= 16) return GemmRoute::kDirect;
  if (small_knob && M <= 2048 && K <= 512) return GemmRoute::kFewRow;
  if (lds_knob && M >= kGemmLdsMinRows) return GemmRoute::kLds;
  return GemmRoute::kKSplit;
}

// an operand whose rows (of every batch) start 16-byte aligned is read with 16-byte loads (AV / BV of the kernels)
static bool vec_ok(const float* p, long long ld, long long stride) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0 && stride % 4 == 0; }

// f(AV, BV) with the two alignment flags as compile-time constants
template <class F>
static void gemm_by_vec(bool av, bool bv, F&& f) {
  if (av && bv) f(std::true_type{}, std::true_type{});
  else if (av) f(std::true_type{}, std::false_type{});
  else if (bv) f(std::false_type{}, std::true_type{});
  else f(std::false_type{}, std::false_type{});
}

// the kernel choice of tgmx_sgemm_nt / tgmx_sgemm_nt_ep (arguments checked by the caller)
static int sgemm_nt_run(const GemmArgs& g, int32_t batch, tgmx_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  const GemmRoute route = gemm_route(g.M, g.K);
  const auto tiles = [&](int bm, int bn) { return dim3((unsigned)((g.M + bm - 1) / bm), (unsigned)((g.N + bn - 1) / bn), (unsigned)batch); };
  gemm_by_vec(vec_ok(g.A, g.lda, g.sA), vec_ok(g.B, g.ldb, g.sB), [&](auto av, auto bv) {
    constexpr bool AV = decltype(av)::value, BV = decltype(bv)::value;
    switch (route) {
      case GemmRoute::kFewRow: {  // the latency-shaped kernel (see sgemm_nt_small_kernel)
        const dim3 sgrid = tiles(32, 32), sblock(512);
        const int steps = (g.K + 127) / 128;
        if (steps == 1) hipLaunchKernelGGL((sgemm_nt_small_kernel<AV, BV, 1>), sgrid, sblock, 0, st, g);
        else if (steps == 2) hipLaunchKernelGGL((sgemm_nt_small_kernel<AV, BV, 2>), sgrid, sblock, 0, st, g);
        else if (steps == 3) hipLaunchKernelGGL((sgemm_nt_small_kernel<AV, BV, 3>), sgrid, sblock, 0, st, g);
        else hipLaunchKernelGGL((sgemm_nt_small_kernel<AV, BV, 4>), sgrid, sblock, 0, st, g);
        break;
      }
      case GemmRoute::kLds: hipLaunchKernelGGL((sgemm_nt_lds_kernel<AV, BV>), tiles(kLdsBM, kLdsBN), dim3(256), 0, st, g); break;
      case GemmRoute::kKSplit: hipLaunchKernelGGL((sgemm_nt_kernel<AV, BV, true, 8>), tiles(32, 64), dim3(256), 0, st, g); break;
      case GemmRoute::kDirect: hipLaunchKernelGGL((sgemm_nt_kernel<AV, BV, false, 8>), tiles(128, 64), dim3(256), 0, st, g); break;
    }
  });
  TGMX_CHECK_LAUNCH(route == GemmRoute::kFewRow ? "sgemm_nt(small)" : route == GemmRoute::kLds ? "sgemm_nt(lds)" : "sgemm_nt");
  return TGMX_OK;
}

extern "C" int tgmx_sgemm_nt(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M,
                             int32_t N, int32_t K, const float* bias, int32_t relu, int32_t batch, int64_t strideA,
                             int64_t strideB, int64_t strideC, tgmx_stream_t stream) {
  TGMX_REQUIRE(M >= 0 && N > 0 && K > 0 && batch > 0, "sgemm_nt: bad sizes M=%lld N=%d K=%d batch=%d", (long long)M, N, K, batch);
  if (M == 0) return TGMX_OK;
  TGMX_REQUIRE(A && B && C, "sgemm_nt: null pointer");
  TGMX_REQUIRE(lda >= K && ldb >= K && ldc >= N, "sgemm_nt: leading dimension smaller than the row length");
  return sgemm_nt_run(GemmArgs{A, B, C, bias, lda, ldb, ldc, strideA, strideB, strideC, M, N, K, relu ? 1 : 0}, batch, stream);
}

extern "C" int tgmx_sgemm_nt_ep(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int32_t N,
                                int32_t K, const float* bias, int32_t act, const float* res, int64_t ldr, tgmx_stream_t stream) {
  TGMX_REQUIRE(M >= 0 && N > 0 && K > 0 && act >= 0 && act <= 2, "sgemm_nt_ep: bad sizes M=%lld N=%d K=%d act=%d", (long long)M, N, K, act);
  if (M == 0) return TGMX_OK;
  TGMX_REQUIRE(A && B && C, "sgemm_nt_ep: null pointer");
  TGMX_REQUIRE(lda >= K && ldb >= K && ldc >= N && (!res || ldr >= N), "sgemm_nt_ep: leading dimension smaller than the row length");
  return sgemm_nt_run(GemmArgs{A, B, C, bias, lda, ldb, ldc, 0, 0, 0, M, N, K, act, res, ldr}, 1, stream);
}

// internal (csrc/tgn.hip): two independent C = A B^T (+ bias) problems as ONE launch.  Each problem goes through the body that
// gemm_route gives it alone, so results never depend on the pairing; the pair kernels instantiate the K-split and the LDS-staged body
// for aligned operands only, so a problem on another route or with an unaligned operand (or TGMX_GEMM_PAIR=0) makes it two launches.
int tgmx_internal_sgemm_nt_pair(const GemmCall& c0, const GemmCall& c1, tgmx_stream_t stream) {
  static const bool pair_knob = [] { const char* e = getenv("TGMX_GEMM_PAIR"); return !(e && e[0] == '0'); }();  // A/B knob
  const GemmCall* cs[2] = {&c0, &c1};
  bool lds[2], pairable = pair_knob;
  for (int q = 0; q < 2; ++q) {
    const GemmCall& c = *cs[q];
    const GemmRoute route = gemm_route(c.M, c.K);
    lds[q] = route == GemmRoute::kLds;
    pairable = pairable && c.M > 0 && c.batch > 0 && (lds[q] || route == GemmRoute::kKSplit) && vec_ok(c.A, c.lda, c.sA) && vec_ok(c.B, c.ldb, c.sB);
  }
  if (!pairable) {
    for (const GemmCall* c : cs)
      if (int rc = tgmx_sgemm_nt(c->A, c->lda, c->B, c->ldb, c->C, c->ldc, c->M, c->N, c->K, c->bias, c->relu, c->batch, c->sA, c->sB, c->sC, stream)) return rc;
    return TGMX_OK;
  }
  GemmPairArgs p;
  unsigned tiles[2];
  for (int q = 0; q < 2; ++q) {
    const GemmCall& c = *cs[q];
    TGMX_REQUIRE(c.A && c.B && c.C && c.N > 0 && c.lda >= c.K && c.ldb >= c.K && c.ldc >= c.N, "sgemm_nt_pair: bad problem %d", q);
    p.g[q] = GemmArgs{c.A, c.B, c.C, c.bias, c.lda, c.ldb, c.ldc, c.sA, c.sB, c.sC, c.M, c.N, c.K, c.relu ? 1 : 0};
    p.ny[q] = (unsigned)((c.N + 63) / 64);
    p.nz[q] = (unsigned)c.batch;
    p.lds[q] = lds[q];
    tiles[q] = (unsigned)(lds[q] ? (c.M + kLdsBM - 1) / kLdsBM : (c.M + 31) / 32);
  }
  p.tiles0 = tiles[0];
  const dim3 grid(tiles[0] + tiles[1], p.ny[0] > p.ny[1] ? p.ny[0] : p.ny[1], p.nz[0] > p.nz[1] ? p.nz[0] : p.nz[1]);
  const bool both = lds[0] && lds[1], mixed = lds[0] != lds[1];  // mixed: each through its own body, still one launch
  hipLaunchKernelGGL((both ? sgemm_nt_lds_pair_kernel : mixed ? sgemm_nt_mixed_pair_kernel : sgemm_nt_pair_kernel), grid, dim3(256), 0, (hipStream_t)stream, p);
  TGMX_CHECK_LAUNCH(both ? "sgemm_nt_pair(lds)" : mixed ? "sgemm_nt_pair(mixed)" : "sgemm_nt_pair");
  return TGMX_OK;
}

extern "C" int tgmx_gather_rows(const float* table, int64_t num_rows, int32_t dim, const int32_t* idx, int64_t n, float* out,
                                int64_t ldo, tgmx_stream_t stream) {
  TGMX_REQUIRE(num_rows > 0 && dim > 0 && n >= 0 && ldo >= dim, "gather_rows: bad sizes");
  if (n == 0) return TGMX_OK;
  TGMX_REQUIRE(table && idx && out, "gather_rows: null pointer");
  long long blocks = (n * dim + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, table, (long long)num_rows,
                     dim, idx, (long long)n, out, (long long)ldo);
  TGMX_CHECK_LAUNCH("gather_rows");
  return TGMX_OK;
}

extern "C" int tgmx_dropout(const float* x, int64_t ldx, int64_t R, int32_t C, const tgmx_dropout_t* drop, float* out, int64_t ldo,
                            tgmx_stream_t stream) {
  TGMX_REQUIRE(R >= 0 && C > 0 && ldx >= C && ldo >= C, "dropout: bad sizes R=%lld C=%d", (long long)R, C);
  if (R == 0) return TGMX_OK;
  TGMX_REQUIRE(x && out, "dropout: null pointer");
  TGMX_REQUIRE(!drop || (drop->p >= 0.f && drop->p < 1.f), "dropout: p must be in [0, 1)");
  long long blocks = (R * C + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(dropout_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, (long long)ldx, (long long)R, C, make_dropout(drop),
                     drop ? (long long)drop->row0 : 0ll, out, (long long)ldo);
  TGMX_CHECK_LAUNCH("dropout");
  return TGMX_OK;
}

extern "C" int tgmx_time2vec(const void* x, int32_t x_is_int64, const float* w, const float* b, int32_t T, int64_t n,
                             float* out, tgmx_stream_t stream) {
  TGMX_REQUIRE(T > 0 && n >= 0, "time2vec: bad sizes");
  if (n == 0) return TGMX_OK;
  TGMX_REQUIRE(x && w && b && out, "time2vec: null pointer");
  long long blocks = (n * T + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  if (x_is_int64)
    hipLaunchKernelGGL(time2vec_kernel<int64_t>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const int64_t*)x, w, b,
                       T, (long long)n, out);
  else
    hipLaunchKernelGGL(time2vec_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)x, w, b, T,
                       (long long)n, out);
  TGMX_CHECK_LAUNCH("time2vec");
  return TGMX_OK;
}

extern "C" int tgmx_layernorm_rows(const float* x, int64_t ldx, int64_t R, int32_t d, const float* gamma, const float* beta, float eps, float* y,
                                   int64_t ldy, tgmx_stream_t stream) {
  TGMX_REQUIRE(R >= 0 && d > 0 && ldx >= d && ldy >= d && (R + 3) / 4 < (1ll << 31), "layernorm_rows: bad sizes R=%lld d=%d", (long long)R, d);
  if (R == 0) return TGMX_OK;
  TGMX_REQUIRE(x && gamma && beta && y, "layernorm_rows: null pointer");
  hipLaunchKernelGGL(layernorm_rows_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, (long long)ldx, (long long)R, d,
                     gamma, beta, eps, y, (long long)ldy);
  TGMX_CHECK_LAUNCH("layernorm_rows");
  return TGMX_OK;
}

struct PackJobs {
  tgmx_pack_job_t job[TGMX_PACK_MAX_JOBS];
};
// blockIdx.y = job; the job's dst elements strided over blockIdx.x
__global__ __launch_bounds__(256) void pack2d_kernel(const PackJobs J) {
  const tgmx_pack_job_t j = J.job[blockIdx.y];
  const long long total = (long long)j.dst_rows * j.dst_cols;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(e / j.dst_cols), c = (int)(e - (long long)r * j.dst_cols);
    float v = 0.f;
    if (r < j.rows && c < j.cols) v = j.transpose ? j.src[(long long)c * j.src_ld + r] : j.src[(long long)r * j.src_ld + c];
    j.dst[(long long)r * j.dst_ld + c] = v;
  }
}

extern "C" int tgmx_pack2d(const tgmx_pack_job_t* jobs, int32_t n_jobs, tgmx_stream_t stream) {
  TGMX_REQUIRE(n_jobs >= 0 && n_jobs <= TGMX_PACK_MAX_JOBS, "pack2d: %d jobs (at most %d per call)", n_jobs, TGMX_PACK_MAX_JOBS);
  if (n_jobs == 0) return TGMX_OK;
  TGMX_REQUIRE(jobs, "pack2d: null pointer");
  PackJobs J{};
  long long most = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const tgmx_pack_job_t& j = jobs[i];
    TGMX_REQUIRE(j.src && j.dst && j.rows >= 0 && j.cols >= 0 && j.dst_rows >= j.rows && j.dst_cols >= j.cols && j.dst_ld >= j.dst_cols &&
                     j.src_ld >= (j.transpose ? j.rows : j.cols),
                 "pack2d: job %d is malformed", i);
    J.job[i] = j;
    const long long total = (long long)j.dst_rows * j.dst_cols;
    most = total > most ? total : most;
  }
  if (most == 0) return TGMX_OK;
  long long bx = (most + 1023) / 1024;  // ~4 elements per thread
  if (bx > 256) bx = 256;
  hipLaunchKernelGGL(pack2d_kernel, dim3((unsigned)bx, (unsigned)n_jobs), dim3(256), 0, (hipStream_t)stream, J);
  TGMX_CHECK_LAUNCH("pack2d");
  return TGMX_OK;
}
