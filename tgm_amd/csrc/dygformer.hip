// DyGFormer (the reference's tgm/nn/encoder/dygformer.py) for gfx950, the forward (inference, and the saving form training takes): the neighbour co-occurrence count and its encoding, the
// prologue that builds the node / edge / time channel inputs straight from the sampler's hop-0 output (through row indices: no gathered
// copy of nbr_edge_x), LayerNorm over token rows, multi-head self-attention over the 2 Np tokens of one (src, dst) pair on the exact-fp32
// MFMA, and the per-side patch mean.  The dense contractions (patch projections, in / out projections, FFN, output layer) run on the
// GEMM of csrc/dense.hip through tgmx_sgemm_nt_ep.
//
// Sequence order everywhere: sequence q = 2 p + side (side 0 = the pair's source, 1 = its destination), slot j of it at row q L + j;
// slot 0 is the seed itself, slot j > 0 the sampler's slot j - 1 of row src_rows[p] / dst_rows[p] (NULL: rows p and P + p).
#include "common.h"
#include "gemm.h"
#include "mha_small.h"

namespace tgmx {

constexpr int kDygMaxL = 2048;  // co-occurrence: both id sequences in LDS (16 KiB)

// the sampler row and the seed of sequence q (row < 0: indices out of range, the sequence is treated as all pads)
struct DygSeqs {
  const int32_t *src, *dst, *src_rows, *dst_rows;
  long long P, S;
};
__device__ __forceinline__ void dyg_seq(const DygSeqs& s, long long q, int32_t& seed, long long& row) {
  const long long p = q >> 1;
  const bool d = q & 1;
  seed = d ? s.dst[p] : s.src[p];
  const int32_t* rows = d ? s.dst_rows : s.src_rows;
  row = rows ? (long long)rows[p] : (d ? s.P + p : p);
  if (row < 0 || row >= s.S) row = -1;
}

// ---- co-occurrence --------------------------------------------------------------------------------------------------------------------

// enc(c) = W2 relu(w1 c + b1) + b2 for every count c = 0 .. L: one workgroup per count, one thread per output channel
__global__ __launch_bounds__(256) void dyg_cotable_kernel(const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                                         const float* __restrict__ b2, int C, float* __restrict__ table) {
  const float c = (float)blockIdx.x;
  for (int o = threadIdx.x; o < C; o += blockDim.x) {
    float a = 0.f;
    for (int j = 0; j < C; ++j) a = __fmaf_rn(w2[(long long)o * C + j], fmaxf(__fmaf_rn(w1[j], c, b1[j]), 0.f), a);
    table[(long long)blockIdx.x * C + o] = a + b2[o];
  }
}

// one workgroup per pair: both id sequences in LDS, every slot counts its id in its own and in the other sequence (pads compare equal to
// each other and are zeroed afterwards)
__global__ void dyg_cooc_kernel(DygSeqs sq, const int32_t* __restrict__ nbr_nids, int k, const float* __restrict__ table, int C,
                                int32_t* __restrict__ counts, float* __restrict__ feat, long long ldf) {
  extern __shared__ int32_t ids[];  // [2][L]
  const int L = k + 1;
  const long long p = blockIdx.x;
  for (int e = threadIdx.x; e < 2 * L; e += blockDim.x) {
    const int side = e >= L, j = e - side * L;
    int32_t seed;
    long long row;
    dyg_seq(sq, 2 * p + side, seed, row);
    ids[e] = j == 0 ? seed : (row < 0 ? -1 : nbr_nids[row * k + j - 1]);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * L; e += blockDim.x) {
    const int side = e >= L;
    const int32_t id = ids[e];
    const int32_t* mine = ids + side * L;
    const int32_t* other = ids + (1 - side) * L;
    int cs = 0, cx = 0;
    for (int j = 0; j < L; ++j) {
      cs += mine[j] == id;
      cx += other[j] == id;
    }
    if (id == -1) cs = cx = 0;
    const long long r = 2 * p * L + e;  // = (2 p + side) L + j
    if (counts) {
      counts[2 * r] = cs;
      counts[2 * r + 1] = cx;
    }
    ids[2 * L + e] = cs | (cx << 16);
  }
  if (!feat) return;
  __syncthreads();
  for (long long e = threadIdx.x; e < 2ll * L * ldf; e += blockDim.x) {
    const int s = (int)(e / ldf), c = (int)(e - s * ldf);
    const int pk = ids[2 * L + s];
    feat[(2 * p * L + s) * ldf + c] = c < C ? table[(long long)(pk & 0xFFFF) * C + c] + table[(long long)(pk >> 16) * C + c] : 0.f;
  }
}

// ---- prologue ---------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void dyg_prologue_kernel(DygSeqs sq, const float* __restrict__ node_x, long long num_nodes, int dN,
                                                          const int64_t* __restrict__ edge_time, const int32_t* __restrict__ nbr_nids,
                                                          const int64_t* __restrict__ nbr_t, const float* __restrict__ nbr_x, int k, int dE,
                                                          const float* __restrict__ tw, const float* __restrict__ tb, int dT,
                                                          float* __restrict__ node_out, int ldn, float* __restrict__ edge_out, int lde,
                                                          float* __restrict__ time_out, int ldt) {
  const int L = k + 1, W = ldn + lde + ldt;
  const long long total = 2 * sq.P * L * W;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
    const long long r = e / W;  // slot row q L + j
    const int c = (int)(e - r * W);
    const long long q = r / L;
    const int j = (int)(r - q * L);
    int32_t seed;
    long long row;
    dyg_seq(sq, q, seed, row);
    const long long slot = row < 0 ? -1 : row * k + j - 1;  // the sampler's slot (j > 0)
    const int32_t id = j == 0 ? seed : (slot < 0 ? -1 : nbr_nids[slot]);
    if (c < ldn) {
      node_out[r * ldn + c] = (c < dN && id >= 0 && id < num_nodes) ? node_x[(long long)id * dN + c] : 0.f;
    } else if (c < ldn + lde) {
      const int ce = c - ldn;
      edge_out[r * lde + ce] = (ce < dE && j > 0 && slot >= 0) ? nbr_x[slot * dE + ce] : 0.f;  // padded slots: as the sampler wrote them
    } else {
      const int ct = c - ldn - lde;
      float v = 0.f;
      if (ct < dT && id != -1) {
        const float dt = (j == 0 || slot < 0) ? 0.f : (float)(edge_time[q >> 1] - nbr_t[slot]);  // int64 difference, then .float()
        v = cosf(__fmaf_rn(dt, tw[ct], tb[ct]));
      }
      time_out[r * ldt + ct] = v;
    }
  }
}

// ---- multi-head self-attention over short sequences ---------------------------------------------------------------------------------------
// One workgroup (4 waves) per (sequence group, head).  LDS: kv [Tp][ldk] holds K, later V; pr [Tp][ldr] holds Q, and row tile by row tile
// is overwritten with the probabilities (a row tile's Q is read by the one wave that owns the tile, which is also the one that writes its
// probabilities).  Scores live in the MFMA accumulators: lane (c, g) of a 16 x 16 tile holds rows 4 g .. 4 g + 3 of column c, so a row's
// max / sum is a reduction over the 16 lanes of a group (xor 1, 2, 4, 8) and over the row tile's column tiles.
// Both leading dimensions are 4 (mod 8) floats: the 16 rows that one MFMA operand load touches fall into 16 different bank quads.
// drop (training): the normalised probabilities are scaled by the site's mask before the P V product, element ((grp H + h) T + i) T + j.
__global__ __launch_bounds__(256) void mha_small_kernel(const float* __restrict__ qkv, long long ldq, int T, int H, int dh, float scale,
                                                       float* __restrict__ out, long long ldo, int ldk, int ldr, const DropoutArgs drop) {
  extern __shared__ float lds[];
  const int Tp = (T + 15) & ~15, nI = Tp >> 4, dh4 = (dh + 3) & ~3, D = H * dh;
  float* __restrict__ kv = lds;
  float* __restrict__ pr = lds + (size_t)Tp * ldk;
  const long long grp = blockIdx.x / H;
  const int h = blockIdx.x % H;
  const float* __restrict__ base = qkv + grp * T * ldq + (long long)h * dh;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, lc = lane & 15, lg = lane >> 4;
  for (int e = tid; e < Tp * ldk; e += 256) {
    const int r = e / ldk, c = e - r * ldk;
    const bool ok = r < T && c < dh;
    kv[e] = ok ? base[(long long)r * ldq + D + c] : 0.f;
    pr[r * ldr + c] = ok ? base[(long long)r * ldq + c] : 0.f;
  }
  __syncthreads();
  for (int i = wave; i < nI; i += 4) {
    floatx4 acc[kMhaJ];
#pragma unroll
    for (int j = 0; j < kMhaJ; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
    const float* __restrict__ qa = pr + (i * 16 + lc) * ldr + lg;
    const float* __restrict__ kb = kv + lc * ldk + lg;
    for (int kk = 0; kk < dh4; kk += 4) {
      const float a = qa[kk];
#pragma unroll
      for (int j = 0; j < kMhaJ; ++j)
        if (j < nI) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, kb[j * 16 * ldk + kk], acc[j], 0, 0, 0);
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
      float* __restrict__ po = pr + (i * 16 + 4 * lg + r) * ldr + lc;
      if (drop.thresh == 0) {
#pragma unroll
        for (int j = 0; j < kMhaJ; ++j)
          if (j < nI) po[j * 16] = acc[j][r] / s;
      } else {
        const int row = i * 16 + 4 * lg + r;
        const unsigned long long e0 = ((unsigned long long)blockIdx.x * T + row) * T + lc;
#pragma unroll
        for (int j = 0; j < kMhaJ; ++j)
          if (j < nI) po[j * 16] = (row < T && j * 16 + lc < T) ? acc[j][r] / s * dropout_scale(drop, e0 + j * 16) : 0.f;
      }
    }
  }
  __syncthreads();  // every wave is done with K
  for (int e = tid; e < Tp * ldk; e += 256) {
    const int r = e / ldk, c = e - r * ldk;
    kv[e] = (r < T && c < dh) ? base[(long long)r * ldq + 2 * D + c] : 0.f;
  }
  __syncthreads();
  const int nN = (dh + 15) >> 4;
  for (int i = wave; i < nI; i += 4) {
    const float* __restrict__ pa = pr + (i * 16 + lc) * ldr + lg;
    for (int n = 0; n < nN; ++n) {
      const int col = n * 16 + lc;
      const bool cok = col < ldk;  // columns [dh, ldk) hold zeros
      const float* __restrict__ vb = kv + lg * ldk + (cok ? col : 0);
      floatx4 o = floatx4{0.f, 0.f, 0.f, 0.f};
      for (int kk = 0; kk < Tp; kk += 4) {
        const float b = cok ? vb[kk * ldk] : 0.f;
        o = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[kk], b, o, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = i * 16 + 4 * lg + r;
        if (row < T && col < dh) out[(grp * T + row) * ldo + (long long)h * dh + col] = o[r];
      }
    }
  }
}

// ---- tail -------------------------------------------------------------------------------------------------------------------------------

// mean over the Np tokens of each side: x rows (2 p + side) Np + t  ->  mean row side P + p (sources first, as the output is returned)
__global__ __launch_bounds__(256) void dyg_mean_kernel(const float* __restrict__ x, long long ldx, long long P, int Np, int D,
                                                      float* __restrict__ mean, long long ldm) {
  const long long q = blockIdx.x;
  const float* __restrict__ xs = x + q * Np * ldx;
  float* __restrict__ o = mean + ((q & 1) * P + (q >> 1)) * ldm;
  for (int c = threadIdx.x; c < ldm; c += blockDim.x) {
    float a = 0.f;
    if (c < D) {
#pragma unroll 4
      for (int t = 0; t < Np; ++t) a += xs[t * ldx + c];
      a /= (float)Np;
    }
    o[c] = a;
  }
}

}  // namespace tgmx

using namespace tgmx;

extern "C" int tgmx_dygformer_cooccurrence(const int32_t* src, const int32_t* dst, int64_t P, const int32_t* nbr_nids, int64_t S, int32_t k,
                                           const int32_t* src_rows, const int32_t* dst_rows, const float* co_w1, const float* co_b1,
                                           const float* co_w2, const float* co_b2, int32_t C, float* table, int32_t* counts, float* feat,
                                           int64_t ldf, tgmx_stream_t stream) {
  TGMX_REQUIRE(P >= 0 && S >= 0 && k >= 0 && k < kDygMaxL, "dygformer_cooccurrence: bad sizes P=%lld S=%lld k=%d (sequences of at most %d slots)",
               (long long)P, (long long)S, k, kDygMaxL);
  if (P == 0) return TGMX_OK;
  TGMX_REQUIRE(src && dst && (k == 0 || S == 0 || nbr_nids) && (counts || feat), "dygformer_cooccurrence: null pointer");
  TGMX_REQUIRE(!feat || (C > 0 && ldf >= C && table && co_w1 && co_b1 && co_w2 && co_b2), "dygformer_cooccurrence: features need the encoder and its table");
  hipStream_t st = (hipStream_t)stream;
  const int L = k + 1;
  if (feat) {
    hipLaunchKernelGGL(dyg_cotable_kernel, dim3((unsigned)(L + 1)), dim3(C <= 64 ? 64 : 256), 0, st, co_w1, co_b1, co_w2, co_b2, C, table);
    TGMX_CHECK_LAUNCH("dygformer_cooccurrence(table)");
  }
  const DygSeqs sq{src, dst, src_rows, dst_rows, (long long)P, (long long)S};
  const int threads = 2 * L <= 64 ? 64 : 256;  // one wave for short sequences
  hipLaunchKernelGGL(dyg_cooc_kernel, dim3((unsigned)P), dim3(threads), sizeof(int32_t) * 4 * L, st, sq, nbr_nids, k, table, C, counts, feat, (long long)ldf);
  TGMX_CHECK_LAUNCH("dygformer_cooccurrence");
  return TGMX_OK;
}

extern "C" int tgmx_dygformer_prologue(const float* node_x, int64_t num_nodes, int32_t dN, const int32_t* src, const int32_t* dst,
                                       const int64_t* edge_time, int64_t P, const int32_t* nbr_nids, const int64_t* nbr_t, const float* nbr_x,
                                       int64_t S, int32_t k, int32_t dE, const int32_t* src_rows, const int32_t* dst_rows, const float* tw,
                                       const float* tb, int32_t dT, float* node_out, int64_t ldn, float* edge_out, int64_t lde, float* time_out,
                                       int64_t ldt, tgmx_stream_t stream) {
  TGMX_REQUIRE(P >= 0 && S >= 0 && k >= 0 && k < kDygMaxL && num_nodes > 0 && dN > 0 && dE > 0 && dT > 0 && ldn >= dN && lde >= dE && ldt >= dT &&
                   ldn + lde + ldt < (1 << 30),
               "dygformer_prologue: bad sizes P=%lld S=%lld k=%d dN=%d dE=%d dT=%d", (long long)P, (long long)S, k, dN, dE, dT);
  if (P == 0) return TGMX_OK;
  TGMX_REQUIRE(node_x && src && dst && edge_time && (k == 0 || S == 0 || (nbr_nids && nbr_t && nbr_x)) && tw && tb && node_out && edge_out && time_out,
               "dygformer_prologue: null pointer");
  const long long total = 2 * P * (k + 1) * (ldn + lde + ldt);
  long long blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  const DygSeqs sq{src, dst, src_rows, dst_rows, (long long)P, (long long)S};
  hipLaunchKernelGGL(dyg_prologue_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, sq, node_x, (long long)num_nodes, dN, edge_time,
                     nbr_nids, nbr_t, nbr_x, k, dE, tw, tb, dT, node_out, (int)ldn, edge_out, (int)lde, time_out, (int)ldt);
  TGMX_CHECK_LAUNCH("dygformer_prologue");
  return TGMX_OK;
}

extern "C" int tgmx_mha_small_train(const float* qkv, int64_t ldq, int64_t B, int32_t T, int32_t H, int32_t dh, float* out, int64_t ldo,
                                    const tgmx_dropout_t* drop, tgmx_stream_t stream) {
  TGMX_REQUIRE(!drop || (drop->p >= 0.f && drop->p < 1.f), "mha_small: p must be in [0, 1)");
  TGMX_REQUIRE(B >= 0 && T > 0 && H > 0 && dh > 0 && (long long)H * dh < (1 << 28) && ldq >= 3ll * H * dh && ldo >= (long long)H * dh &&
                   B * H < (1ll << 31),
               "mha_small: bad sizes B=%lld T=%d H=%d dh=%d", (long long)B, T, H, dh);
  const int Tp = (T + 15) & ~15, ldk = mha_ld((dh + 3) & ~3), ldp = mha_ld(Tp), ldr = ldk > ldp ? ldk : ldp;
  const size_t lds = sizeof(float) * (size_t)Tp * (ldk + ldr);
  if (T > kMhaMaxT || dh > kMhaMaxDh || lds > kMhaMaxLds) {
    set_error("mha_small: T=%d tokens x head dimension %d is outside the native envelope (T <= %d, dh <= %d)", T, dh, kMhaMaxT, kMhaMaxDh);
    return TGMX_E_UNSUPPORTED;
  }
  if (B == 0) return TGMX_OK;
  TGMX_REQUIRE(qkv && out, "mha_small: null pointer");
  if (lds > 64 * 1024) {  // past the default limit of a launch; set per call: the attribute belongs to the current device
    const hipError_t attr = hipFuncSetAttribute((const void*)mha_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMhaMaxLds);
    if (attr != hipSuccess) {
      (void)hipGetLastError();
      set_error("mha_small: T=%d x dh=%d needs %zu bytes of LDS and the limit cannot be raised: %s", T, dh, lds, hipGetErrorString(attr));
      return TGMX_E_UNSUPPORTED;
    }
  }
  hipLaunchKernelGGL(mha_small_kernel, dim3((unsigned)(B * H)), dim3(256), lds, (hipStream_t)stream, qkv, (long long)ldq, T, H, dh,
                     1.f / sqrtf((float)dh), out, (long long)ldo, ldk, ldr, make_dropout(drop));
  TGMX_CHECK_LAUNCH("mha_small");
  return TGMX_OK;
}

extern "C" int tgmx_mha_small(const float* qkv, int64_t ldq, int64_t B, int32_t T, int32_t H, int32_t dh, float* out, int64_t ldo,
                              tgmx_stream_t stream) {
  return tgmx_mha_small_train(qkv, ldq, B, T, H, dh, out, ldo, nullptr, stream);
}

extern "C" int tgmx_dygformer_tail(const float* x, int64_t ldx, int64_t P, int32_t Np, int32_t D, float* mean, int64_t ldm, const float* out_w,
                                   const float* out_b, int32_t E, float* out, tgmx_stream_t stream) {
  TGMX_REQUIRE(P >= 0 && Np > 0 && D > 0 && E > 0 && ldx >= D && ldm >= D && 2 * P < (1ll << 31), "dygformer_tail: bad sizes P=%lld Np=%d D=%d E=%d",
               (long long)P, Np, D, E);
  if (P == 0) return TGMX_OK;
  TGMX_REQUIRE(x && mean && out_w && out, "dygformer_tail: null pointer");
  hipLaunchKernelGGL(dyg_mean_kernel, dim3((unsigned)(2 * P)), dim3(D <= 64 ? 64 : 256), 0, (hipStream_t)stream, x, (long long)ldx, (long long)P, Np, D,
                     mean, (long long)ldm);
  TGMX_CHECK_LAUNCH("dygformer_tail");
  return tgmx_sgemm_nt_ep(mean, ldm, out_w, D, out, E, 2 * P, E, D, out_b, 0, nullptr, 0, stream);
}

// one transformer layer x_in -> x_out [R, ldx] (x_out may be x_in; y, x1, att [R, ldx], qkv [R, ldq], h [R, ldh] scratch).  drop: the
// layer's four sites draw from stream + 0 .. 3; with dropout the three row sites are extra launches (tgmx_dropout in place, tgmx_add_cols)
extern "C" int tgmx_dygformer_layer_train(const tgmx_dygformer_layer_t* ly, int64_t B, int32_t T, int32_t H, int32_t D, float eps,
                                          const float* x_in, float* x_out, float* y, float* x1, float* att, int64_t ldx, float* qkv,
                                          int64_t ldq, float* h, int64_t ldh, const tgmx_dropout_t* drop, tgmx_stream_t stream) {
  TGMX_REQUIRE(ly && B >= 0 && T > 0 && H > 0 && D > 0 && D % H == 0 && ldx >= D && ldq >= 3ll * D && ldh >= 4ll * D && ldx % 4 == 0 && ldq % 4 == 0 &&
                   ldh % 4 == 0,
               "dygformer_layer: bad sizes B=%lld T=%d H=%d D=%d (leading dimensions: multiples of 4)", (long long)B, T, H, D);
  TGMX_REQUIRE(!drop || (drop->p >= 0.f && drop->p < 1.f), "dygformer_layer: p must be in [0, 1)");
  const long long R = B * T;
  const bool dropping = drop && drop->p > 0.f;
  tgmx_dropout_t site[4];
  for (int s = 0; s < 4; ++s) site[s] = dropping ? tgmx_dropout_t{drop->p, drop->seed, drop->stream + s, 0} : tgmx_dropout_t{0.f, 0, 0, 0};
  int rc;
  if ((rc = tgmx_layernorm_rows(x_in, ldx, R, D, ly->ln0_g, ly->ln0_b, eps, y, ldx, stream))) return rc;
  if ((rc = tgmx_sgemm_nt_ep(y, ldx, ly->in_w, D, qkv, ldq, R, 3 * D, D, ly->in_b, 0, nullptr, 0, stream))) return rc;
  if ((rc = tgmx_mha_small_train(qkv, ldq, B, T, H, D / H, att, ldx, &site[0], stream))) return rc;
  if (!dropping) {
    if ((rc = tgmx_sgemm_nt_ep(att, ldx, ly->out_w, D, x1, ldx, R, D, D, ly->out_b, 0, x_in, ldx, stream))) return rc;
  } else {
    if ((rc = tgmx_sgemm_nt_ep(att, ldx, ly->out_w, D, x1, ldx, R, D, D, ly->out_b, 0, nullptr, 0, stream))) return rc;
    if ((rc = tgmx_dropout(x1, ldx, R, D, &site[1], x1, ldx, stream))) return rc;
    if ((rc = tgmx_add_cols(x1, ldx, x_in, ldx, R, D, 1, stream))) return rc;
  }
  if ((rc = tgmx_layernorm_rows(x1, ldx, R, D, ly->ln1_g, ly->ln1_b, eps, y, ldx, stream))) return rc;
  if ((rc = tgmx_sgemm_nt_ep(y, ldx, ly->w1, D, h, ldh, R, 4 * D, D, ly->b1, 2, nullptr, 0, stream))) return rc;
  if (!dropping) return tgmx_sgemm_nt_ep(h, ldh, ly->w2, 4 * D, x_out, ldx, R, D, 4 * D, ly->b2, 0, x1, ldx, stream);
  if ((rc = tgmx_dropout(h, ldh, R, 4 * D, &site[2], h, ldh, stream))) return rc;
  if ((rc = tgmx_sgemm_nt_ep(h, ldh, ly->w2, 4 * D, x_out, ldx, R, D, 4 * D, ly->b2, 0, nullptr, 0, stream))) return rc;
  if ((rc = tgmx_dropout(x_out, ldx, R, D, &site[3], x_out, ldx, stream))) return rc;
  return tgmx_add_cols(x_out, ldx, x1, ldx, R, D, 1, stream);
}

// one transformer layer on x [R, ldx] (in place; y, x1, att [R, ldx], qkv [R, ldq], h [R, ldh] scratch)
extern "C" int tgmx_dygformer_layer(const tgmx_dygformer_layer_t* ly, int64_t B, int32_t T, int32_t H, int32_t D, float eps, float* x, float* y,
                                    float* x1, float* att, int64_t ldx, float* qkv, int64_t ldq, float* h, int64_t ldh, tgmx_stream_t stream) {
  return tgmx_dygformer_layer_train(ly, B, T, H, D, eps, x, x, y, x1, att, ldx, qkv, ldq, h, ldh, nullptr, stream);
}

// save == NULL: inference (every layer in place on a->x, scratch reused).  Otherwise the saving form: counts written, layer l reads its
// input from save->x + l R ldx and writes save->x + (l + 1) R ldx; qkv, att and x1 of layer l stay in save->{qkv, att, x1} + l R ld.
static int dyg_forward(const tgmx_dygformer_fwd_t* a, const tgmx_dygformer_save_t* save, const tgmx_dropout_t* drop, tgmx_stream_t stream) {
  TGMX_REQUIRE(a && a->num_layers >= 0 && a->num_layers <= TGMX_DYGFORMER_MAX_LAYERS, "dygformer_forward: bad argument block");
  TGMX_REQUIRE(a->patch > 0 && a->k >= 0 && (a->k + 1) % a->patch == 0 && a->C > 0 && a->heads > 0 && (4 * a->C) % a->heads == 0,
               "dygformer_forward: bad shape k=%d patch=%d C=%d heads=%d", a->k, a->patch, a->C, a->heads);
  TGMX_REQUIRE(a->ldch[0] % 4 == 0 && a->ldch[1] % 4 == 0 && a->ldch[2] % 4 == 0 && a->ldch[3] % 4 == 0 && a->ldx % 4 == 0,
               "dygformer_forward: leading dimensions must be multiples of 4");
  const long long P = a->P;
  if (P == 0) return TGMX_OK;
  const int L = a->k + 1, Np = L / a->patch, C = a->C, D = 4 * C;
  const long long R = 2 * P * Np;
  int rc;
  TGMX_REQUIRE(!save || (save->counts && save->x && (a->num_layers == 0 || (save->qkv && save->att && save->x1))), "dygformer_forward_train: null save buffer");
  float* x0 = save ? save->x : a->x;
  if ((rc = tgmx_dygformer_cooccurrence(a->src, a->dst, P, a->nbr_nids, a->S, a->k, a->src_rows, a->dst_rows, a->co_w1, a->co_b1, a->co_w2, a->co_b2,
                                        C, a->table, save ? save->counts : nullptr, a->ch[3], a->ldch[3], stream)))
    return rc;
  if ((rc = tgmx_dygformer_prologue(a->node_x, a->num_nodes, a->dN, a->src, a->dst, a->edge_time, P, a->nbr_nids, a->nbr_t, a->nbr_x, a->S, a->k,
                                    a->dE, a->src_rows, a->dst_rows, a->tw, a->tb, a->dT, a->ch[0], a->ldch[0], a->ch[1], a->ldch[1], a->ch[2],
                                    a->ldch[2], stream)))
    return rc;
  // patching is a view: [2 P L, ld] = [2 P Np, patch ld]; channel c's projection writes columns [c C, (c + 1) C) of the token matrix
  for (int c = 0; c < 4; ++c) {
    const long long Kc = (long long)a->patch * a->ldch[c];
    if ((rc = tgmx_sgemm_nt_ep(a->ch[c], Kc, a->proj_w[c], Kc, x0 + (long long)c * C, a->ldx, R, C, (int)Kc, a->proj_b[c], 0, nullptr, 0, stream)))
      return rc;
  }
  if (!save) {
    for (int l = 0; l < a->num_layers; ++l)
      if ((rc = tgmx_dygformer_layer(&a->layers[l], P, 2 * Np, a->heads, D, a->eps, a->x, a->y, a->x1, a->att, a->ldx, a->qkv, a->ldq, a->h, a->ldh,
                                     stream)))
        return rc;
    return tgmx_dygformer_tail(a->x, a->ldx, P, Np, D, a->mean, a->ldx, a->out_w, a->out_b, a->E, a->out, stream);
  }
  const bool dropping = drop && drop->p > 0.f;
  for (int l = 0; l < a->num_layers; ++l) {
    const long long ox = (long long)l * R * a->ldx, oq = (long long)l * R * a->ldq;
    tgmx_dropout_t d{0.f, 0, 0, 0};
    if (dropping) d = tgmx_dropout_t{drop->p, drop->seed, drop->stream + 4ull * l, 0};
    if ((rc = tgmx_dygformer_layer_train(&a->layers[l], P, 2 * Np, a->heads, D, a->eps, save->x + ox, save->x + ox + R * a->ldx, a->y, save->x1 + ox,
                                         save->att + ox, a->ldx, save->qkv + oq, a->ldq, a->h, a->ldh, &d, stream)))
      return rc;
  }
  return tgmx_dygformer_tail(save->x + (long long)a->num_layers * R * a->ldx, a->ldx, P, Np, D, a->mean, a->ldx, a->out_w, a->out_b, a->E, a->out, stream);
}

extern "C" int tgmx_dygformer_forward(const tgmx_dygformer_fwd_t* a, tgmx_stream_t stream) { return dyg_forward(a, nullptr, nullptr, stream); }

extern "C" int tgmx_dygformer_forward_train(const tgmx_dygformer_fwd_t* a, const tgmx_dygformer_save_t* save, const tgmx_dropout_t* drop,
                                            tgmx_stream_t stream) {
  TGMX_REQUIRE(save, "dygformer_forward_train: null save block");
  TGMX_REQUIRE(!drop || (drop->p >= 0.f && drop->p < 1.f), "dygformer_forward_train: p must be in [0, 1)");
  if (a && a->P > 0 && a->patch > 0 && a->heads > 0 && !tgmx_mha_small_train_supported(2 * ((a->k + 1) / a->patch), 4 * a->C / a->heads)) {
    set_error("dygformer_forward_train: %d tokens x head dimension %d is outside the attention backward's envelope", 2 * ((a->k + 1) / a->patch),
              4 * a->C / a->heads);
    return TGMX_E_UNSUPPORTED;
  }
  return dyg_forward(a, save, drop, stream);
}
