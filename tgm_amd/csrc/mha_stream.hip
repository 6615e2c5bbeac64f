// Multi-head self-attention over LONG token sequences (128 < T <= 4096, dh <= 128) for gfx950, forward and backward: the function
// tgmx_mha_small computes -- softmax_j(Q_i . K_j / sqrt(dh)) V per (group b, head h), Q | K | V column blocks of qkv [B T, ldq] -- with K and
// V streamed through LDS in blocks, so nothing T x T is resident or written (flash-attention style: running maximum and sum per query row,
// the output accumulators rescaled when the maximum moves, one division at the end).  Exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) throughout.
//
// Operand layout.  Lane (lc, lg) = (lane & 15, lane >> 4) of a 16 x 16 x 4 MFMA supplies A[row lc][k lg] and B[k lg][col lc] and holds
// C[rows 4 lg .. 4 lg + 3][col lc].  A contraction is a sum over k in any order, so a chunk of 16 k is dealt as "lane group lg takes
// k = 16 c + 4 lg + t at step t" for BOTH operands: an operand stored by rows (Q, K, dO, V in the score products; the P strip) is then
// read as ONE 16-byte LDS read per 4 MFMAs (ds_read_b128 at [row lc][16 c + 4 lg]), and an operand contracted over its rows (V, K, Q, dO
// in the output products) as 4-byte reads at [16 c + 4 lg + t][16 n + lc], consecutive lanes on consecutive banks.
// Pitches: operand blocks [rows][LD], LD = 16 NT + 4 floats (NT = ceil(dh / 16); 4 (mod 8): the four lane groups of a 4-byte column read
// sit 4 rows apart = 16 banks, and 16 rows of a 16-byte row read fall on distinct bank quads); strips [16][block + 4].
//
// Forward: one workgroup of four waves per (b, h, 64 query rows); a wave owns a 16-row tile.  Its Q tile is loaded ONCE, straight into
// registers in operand layout (16 lanes x 64-byte row segments), so Q takes no LDS and is not re-read per key block.  K and V pass
// through LDS in blocks of 64 keys; block n + 1's global loads are issued into registers before block n's MFMAs and stored after them.
// Per block and wave: S = Q K^T (4 score tiles), the row maximum and the rescale, p = exp(s - m) written (dropout mask applied) to the
// wave's P strip, read back once in operand layout (4 x 16-byte reads), and all NT output tiles accumulated from it.  Keys past T are
// excluded from the maximum and the sum and contribute p = 0 exactly.  LDS: (2 . 64 . LD + 4 . 16 . 68) floats = 51 KiB at dh <= 64
// (three workgroups a CU by LDS), 75 KiB at dh = 100 (two), 83 KiB at dh = 128 (one).
//
// Backward: delta = rowsum(dO o O) (one launch), then ONE kernel template in two roles.  A workgroup owns 64 rows (a wave 16 of them) whose
// two operands stay in registers, and streams the other side through LDS in blocks of 32 rows:
//   role KEYS  (own K_w, V_w; stream Q, dO):  X = K_w Q^T = S^T, Y = V_w dO^T = dP^T;  dV_w += (P o m)^T dO,  dK_w += scale dS^T Q
//   role QUERY (own Q_w, dO_w; stream K, V):  X = Q_w K^T = S,   Y = dO_w V^T = dP;    dQ_w += scale dS K
// with P = exp(scale S - lse) (no second softmax), m the regenerated dropout mask, dS = P o (dP o m - delta).  dS (and P o m) go through
// a per-wave LDS strip to turn accumulator layout into operand layout.  Every output element belongs to one wave: written once, no
// atomics, a fixed summation order -- equal bits run to run.
#include "common.h"
#include "gemm.h"
#include "mha_small.h"

namespace tgmx {

constexpr int kStreamMaxT = 4096;  // 2 x the 2048 slots a sequence may have
constexpr int kStreamRows = 64;    // rows a workgroup owns (16 per wave)
constexpr int kStreamBk = 64;      // keys per streamed block, forward
constexpr int kStreamBb = 32;      // rows per streamed block, backward

__device__ __forceinline__ floatx4 mfma4(float a, float b, floatx4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// rows [row0 + lc] of a [T, ld] matrix in A-operand layout: v[c][t] = M[row][16 c + 4 lg + t], zero outside T x dh
template <int NT>
__device__ __forceinline__ void load_own(const float* __restrict__ base, long long ld, int row, int T, int dh, int lg, floatx4 (&v)[NT]) {
  const float* __restrict__ src = base + (long long)row * ld;
#pragma unroll
  for (int c = 0; c < NT; ++c)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int col = 16 * c + 4 * lg + t;
      v[c][t] = (row < T && col < dh) ? src[col] : 0.f;
    }
}

template <int NT>
__global__ __launch_bounds__(256) void mha_stream_fwd_kernel(const float* __restrict__ qkv, long long ldq, int T, int H, int dh, int nQB, float scale,
                                                            float* __restrict__ out, long long ldo, float* __restrict__ lse,
                                                            const DropoutArgs drop) {
  constexpr int W = 16 * NT, LD = W + 4, LDP = kStreamBk + 4, PER = kStreamBk * W / 256;
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, lc = lane & 15, lg = lane >> 4;
  float* __restrict__ Ks = lds;
  float* __restrict__ Vs = Ks + kStreamBk * LD;
  float* __restrict__ Pw = Vs + kStreamBk * LD + wave * 16 * LDP;
  const int qb = blockIdx.x % nQB, D = H * dh;
  const long long bh = blockIdx.x / nQB, grp = bh / H;
  const int h = (int)(bh % H);
  const float* __restrict__ base = qkv + grp * T * ldq + (long long)h * dh;
  const int q0 = qb * kStreamRows + wave * 16;
  const bool active = q0 < T;  // (wave-uniform; an idle wave still stages K and V and meets every barrier)
  floatx4 q[NT], o[NT];
  load_own<NT>(base, ldq, q0 + lc, T, dh, lg, q);
#pragma unroll
  for (int n = 0; n < NT; ++n) o[n] = floatx4{0.f, 0.f, 0.f, 0.f};
  float m[4], l[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) m[r] = -INFINITY, l[r] = 0.f;

  float kreg[PER], vreg[PER];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + 256 * u, r = e / W, c = e - r * W;
      const bool ok = k0 + r < T && c < dh;
      const float* __restrict__ p = base + (long long)(k0 + r) * ldq + c;
      kreg[u] = ok ? p[D] : 0.f;
      vreg[u] = ok ? p[2 * D] : 0.f;
    }
  };
  fetch(0);
  const int nKB = (T + kStreamBk - 1) / kStreamBk;
  for (int kb = 0; kb < nKB; ++kb) {
    __syncthreads();  // the previous block's readers are done
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + 256 * u, r = e / W, c = e - r * W;
      Ks[r * LD + c] = kreg[u];
      Vs[r * LD + c] = vreg[u];
    }
    __syncthreads();
    if (kb + 1 < nKB) fetch((kb + 1) * kStreamBk);  // in flight under this block's MFMAs
    const int k0 = kb * kStreamBk, nv = T - k0 < kStreamBk ? T - k0 : kStreamBk, nj = (nv + 15) >> 4;
    if (active) {
      floatx4 s[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[j] = floatx4{0.f, 0.f, 0.f, 0.f};
        if (j < nj) {
          const float* __restrict__ kp = Ks + (j * 16 + lc) * LD + 4 * lg;
#pragma unroll
          for (int c = 0; c < NT; ++c) {
            const floatx4 kf = *reinterpret_cast<const floatx4*>(kp + 16 * c);
#pragma unroll
            for (int t = 0; t < 4; ++t) s[j] = mfma4(q[c][t], kf[t], s[j]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float mx = m[r];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s[j][r] *= scale;
          if (j * 16 + lc < nv) mx = fmaxf(mx, s[j][r]);
        }
#pragma unroll
        for (int x = 8; x > 0; x >>= 1) mx = fmaxf(mx, __shfl_xor(mx, x));
        const float alpha = m[r] == -INFINITY ? 0.f : expf(m[r] - mx);  // the maximum moved: rescale what was accumulated under the old one
        m[r] = mx;
        l[r] *= alpha;
#pragma unroll
        for (int n = 0; n < NT; ++n) o[n][r] *= alpha;
        const int row = q0 + 4 * lg + r;
        const unsigned long long e0 = ((unsigned long long)bh * T + row) * T + k0 + lc;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < nj) {
            const bool ok = j * 16 + lc < nv;
            float p = ok ? expf(s[j][r] - mx) : 0.f;
            l[r] += p;  // (this lane's columns; the 16 lanes of the row are summed once, at the end)
            if (drop.thresh != 0 && ok && row < T) p *= dropout_scale(drop, e0 + j * 16);
            Pw[(4 * lg + r) * LDP + j * 16 + lc] = p;
          }
      }
    }
    __syncthreads();  // the strip is written (accumulator layout) ...
    if (active) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < nj) {
          const floatx4 pf = *reinterpret_cast<const floatx4*>(Pw + lc * LDP + 16 * c + 4 * lg);  // ... and read once, in operand layout
          const float* __restrict__ vp = Vs + (16 * c + 4 * lg) * LD + lc;
#pragma unroll
          for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int t = 0; t < 4; ++t) o[n] = mfma4(pf[t], vp[t * LD + n * 16], o[n]);
        }
    }
  }
  if (!active) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float lt = l[r];
#pragma unroll
    for (int x = 8; x > 0; x >>= 1) lt += __shfl_xor(lt, x);
    const int row = q0 + 4 * lg + r;
    if (row >= T) continue;
    float* __restrict__ po = out + (grp * T + row) * ldo + (long long)h * dh;
#pragma unroll
    for (int n = 0; n < NT; ++n)
      if (n * 16 + lc < dh) po[n * 16 + lc] = o[n][r] / lt;
    if (lse && lc == 0) lse[bh * T + row] = m[r] + logf(lt);
  }
}

// delta[b, h, i] = sum_c datt[b T + i, h dh + c] att[b T + i, h dh + c]: 16 lanes per (row, head), a fixed order
__global__ __launch_bounds__(256) void mha_stream_delta_kernel(const float* __restrict__ att, const float* __restrict__ datt, long long ldo,
                                                              long long groups, int T, int H, int dh, float* __restrict__ delta) {
  const long long g = ((long long)blockIdx.x * 256 + threadIdx.x) >> 4;
  if (g >= groups) return;  // (a group of 16 lanes leaves together)
  const int lc = threadIdx.x & 15;
  const long long row = g / H;
  const int h = (int)(g % H);
  const long long p = row * ldo + (long long)h * dh;
  float acc = 0.f;
  for (int c = lc; c < dh; c += 16) acc = __fmaf_rn(datt[p + c], att[p + c], acc);
#pragma unroll
  for (int x = 8; x > 0; x >>= 1) acc += __shfl_xor(acc, x);
  if (lc == 0) delta[((row / T) * H + h) * T + row % T] = acc;
}

template <int NT, bool KEYS>
__global__ __launch_bounds__(256) void mha_stream_bwd_kernel(const float* __restrict__ qkv, long long ldq, const float* __restrict__ datt, long long ldo,
                                                            const float* __restrict__ lse, const float* __restrict__ delta, int T, int H, int dh,
                                                            int nOB, float scale, float* __restrict__ dqkv, const DropoutArgs drop) {
  constexpr int W = 16 * NT, LD = W + 4, LDP = kStreamBb + 4, PER = kStreamBb * W / 256, NS = KEYS ? 2 : 1;
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, lc = lane & 15, lg = lane >> 4;
  float* __restrict__ As = lds;
  float* __restrict__ Bs = As + kStreamBb * LD;
  float* __restrict__ DSw = Bs + kStreamBb * LD + wave * NS * 16 * LDP;
  float* __restrict__ PMw = DSw + 16 * LDP;  // (KEYS only)
  const int ob = blockIdx.x % nOB, D = H * dh;
  const long long bh = blockIdx.x / nOB, grp = bh / H;
  const int h = (int)(bh % H);
  const float* __restrict__ qb = qkv + grp * T * ldq + (long long)h * dh;
  const float* __restrict__ db = datt + grp * T * ldo + (long long)h * dh;
  // own: (K, V) or (Q, dO); streamed: (Q, dO) or (K, V)
  const float* __restrict__ sa = KEYS ? qb : qb + D;
  const float* __restrict__ sb = KEYS ? db : qb + 2 * D;
  const long long ldsb = KEYS ? ldo : ldq;
  const int own0 = ob * kStreamRows + wave * 16;
  const bool active = own0 < T;
  floatx4 a[NT], b[NT], g1[NT], g2[KEYS ? NT : 1];
  load_own<NT>(KEYS ? qb + D : qb, ldq, own0 + lc, T, dh, lg, a);
  load_own<NT>(KEYS ? qb + 2 * D : db, KEYS ? ldq : ldo, own0 + lc, T, dh, lg, b);
#pragma unroll
  for (int n = 0; n < NT; ++n) g1[n] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int n = 0; n < (KEYS ? NT : 1); ++n) g2[n] = floatx4{0.f, 0.f, 0.f, 0.f};
  const float* __restrict__ lse_h = lse + bh * T;
  const float* __restrict__ del_h = delta + bh * T;
  float lse_r[4], del_r[4];  // QUERY: the own rows' statistics
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = own0 + 4 * lg + r;
    const bool ok = !KEYS && row < T;
    lse_r[r] = ok ? lse_h[row] : 0.f;
    del_r[r] = ok ? del_h[row] : 0.f;
  }
  const int nSB = (T + kStreamBb - 1) / kStreamBb;
  for (int sbk = 0; sbk < nSB; ++sbk) {
    const int s0 = sbk * kStreamBb;
    __syncthreads();  // the previous block's readers are done
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + 256 * u, r = e / W, c = e - r * W;
      const bool ok = s0 + r < T && c < dh;
      As[r * LD + c] = ok ? sa[(long long)(s0 + r) * ldq + c] : 0.f;
      Bs[r * LD + c] = ok ? sb[(long long)(s0 + r) * ldsb + c] : 0.f;
    }
    __syncthreads();
    if (active) {
      floatx4 x[2], y[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        x[j] = y[j] = floatx4{0.f, 0.f, 0.f, 0.f};
        const float* __restrict__ ap = As + (j * 16 + lc) * LD + 4 * lg;
        const float* __restrict__ bp = Bs + (j * 16 + lc) * LD + 4 * lg;
#pragma unroll
        for (int c = 0; c < NT; ++c) {
          const floatx4 af = *reinterpret_cast<const floatx4*>(ap + 16 * c);
          const floatx4 bf = *reinterpret_cast<const floatx4*>(bp + 16 * c);
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            x[j] = mfma4(a[c][t], af[t], x[j]);
            y[j] = mfma4(b[c][t], bf[t], y[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int st = s0 + j * 16 + lc;  // the streamed row this lane's column stands for
        float lse_c = 0.f, del_c = 0.f;
        if (KEYS && st < T) lse_c = lse_h[st], del_c = del_h[st];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int own = own0 + 4 * lg + r;
          const bool ok = own < T && st < T;
          const int qi = KEYS ? st : own, kj = KEYS ? own : st;
          const float p = ok ? expf(x[j][r] * scale - (KEYS ? lse_c : lse_r[r])) : 0.f;
          const float mk = (drop.thresh != 0 && ok) ? dropout_scale(drop, ((unsigned long long)bh * T + qi) * T + kj) : 1.f;
          DSw[(4 * lg + r) * LDP + j * 16 + lc] = p * (y[j][r] * mk - (KEYS ? del_c : del_r[r]));
          if (KEYS) PMw[(4 * lg + r) * LDP + j * 16 + lc] = p * mk;
        }
      }
    }
    __syncthreads();  // the strips are written (accumulator layout), read back in operand layout
    if (active) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const floatx4 df = *reinterpret_cast<const floatx4*>(DSw + lc * LDP + 16 * c + 4 * lg);
        const float* __restrict__ ap = As + (16 * c + 4 * lg) * LD + lc;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
          for (int t = 0; t < 4; ++t) g1[n] = mfma4(df[t], ap[t * LD + n * 16], g1[n]);
        if (KEYS) {
          const floatx4 pf = *reinterpret_cast<const floatx4*>(PMw + lc * LDP + 16 * c + 4 * lg);
          const float* __restrict__ bp = Bs + (16 * c + 4 * lg) * LD + lc;
#pragma unroll
          for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int t = 0; t < 4; ++t) g2[n] = mfma4(pf[t], bp[t * LD + n * 16], g2[n]);
        }
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = own0 + 4 * lg + r;
    if (row >= T) continue;
    float* __restrict__ po = dqkv + (grp * T + row) * ldq + (long long)h * dh + (KEYS ? D : 0);
#pragma unroll
    for (int n = 0; n < NT; ++n)
      if (n * 16 + lc < dh) {
        po[n * 16 + lc] = g1[n][r] * scale;
        if (KEYS) po[D + n * 16 + lc] = g2[n][r];
      }
  }
}

static size_t stream_fwd_lds(int NT) { return sizeof(float) * (size_t)(2 * kStreamBk * (16 * NT + 4) + 4 * 16 * (kStreamBk + 4)); }
static size_t stream_bwd_lds(int NT, bool keys) { return sizeof(float) * (size_t)(2 * kStreamBb * (16 * NT + 4) + 4 * (keys ? 2 : 1) * 16 * (kStreamBb + 4)); }

// a launch past the default 64 KiB of dynamic LDS raises the kernel's limit first (per call: the attribute belongs to the current device)
static bool raise_lds(const void* fn, size_t bytes) {
  if (bytes <= 64 * 1024) return true;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess) return true;
  (void)hipGetLastError();
  return false;
}

#define TGMX_STREAM_NT(nt, CASE) \
  switch (nt) {                  \
    case 1: CASE(1); break;      \
    case 2: CASE(2); break;      \
    case 3: CASE(3); break;      \
    case 4: CASE(4); break;      \
    case 5: CASE(5); break;      \
    case 6: CASE(6); break;      \
    case 7: CASE(7); break;      \
    default: CASE(8); break;     \
  }

static bool stream_sizes_ok(int64_t B, int T, int H, int dh, int64_t ldq, int64_t ldo) {
  return B >= 0 && T > 0 && H > 0 && dh > 0 && (long long)H * dh < (1 << 28) && ldq >= 3ll * H * dh && ldo >= (long long)H * dh &&
         B * H < (1ll << 31) && B * H * ((T + 15) / 16) < (1ll << 31);
}

}  // namespace tgmx

using namespace tgmx;

extern "C" int tgmx_mha_stream_supported(int32_t T, int32_t dh) { return T > kMhaMaxT && T <= kStreamMaxT && dh >= 1 && dh <= kMhaMaxDh ? 1 : 0; }

extern "C" int tgmx_mha_stream_train(const float* qkv, int64_t ldq, int64_t B, int32_t T, int32_t H, int32_t dh, float* out, int64_t ldo, float* lse,
                                     const tgmx_dropout_t* drop, tgmx_stream_t stream) {
  TGMX_REQUIRE(!drop || (drop->p >= 0.f && drop->p < 1.f), "mha_stream: p must be in [0, 1)");
  TGMX_REQUIRE(stream_sizes_ok(B, T, H, dh, ldq, ldo), "mha_stream: bad sizes B=%lld T=%d H=%d dh=%d", (long long)B, T, H, dh);
  if (!tgmx_mha_stream_supported(T, dh)) {
    set_error("mha_stream: T=%d tokens x head dimension %d is outside the streaming envelope (%d < T <= %d, dh <= %d)", T, dh, kMhaMaxT, kStreamMaxT,
              kMhaMaxDh);
    return TGMX_E_UNSUPPORTED;
  }
  if (B == 0) return TGMX_OK;
  TGMX_REQUIRE(qkv && out, "mha_stream: null pointer");
  const int NT = (dh + 15) / 16, nQB = (T + kStreamRows - 1) / kStreamRows;
  const size_t bytes = stream_fwd_lds(NT);
  const float scale = 1.f / sqrtf((float)dh);
  const DropoutArgs da = make_dropout(drop);
#define CASE(N)                                                                                                                               \
  do {                                                                                                                                        \
    if (!raise_lds((const void*)mha_stream_fwd_kernel<N>, bytes)) {                                                                           \
      set_error("mha_stream: head dimension %d needs %zu bytes of LDS and the limit cannot be raised", dh, bytes);                            \
      return TGMX_E_UNSUPPORTED;                                                                                                              \
    }                                                                                                                                         \
    hipLaunchKernelGGL(mha_stream_fwd_kernel<N>, dim3((unsigned)(B * H * nQB)), dim3(256), bytes, (hipStream_t)stream, qkv, (long long)ldq, T, H, dh, nQB, \
                       scale, out, (long long)ldo, lse, da);                                                                                  \
  } while (0)
  TGMX_STREAM_NT(NT, CASE)
#undef CASE
  TGMX_CHECK_LAUNCH("mha_stream");
  return TGMX_OK;
}

extern "C" int tgmx_mha_stream(const float* qkv, int64_t ldq, int64_t B, int32_t T, int32_t H, int32_t dh, float* out, int64_t ldo,
                               tgmx_stream_t stream) {
  return tgmx_mha_stream_train(qkv, ldq, B, T, H, dh, out, ldo, nullptr, nullptr, stream);
}

extern "C" int tgmx_mha_stream_backward(const float* qkv, int64_t ldq, const float* att, const float* datt, int64_t ldo, const float* lse, int64_t B,
                                        int32_t T, int32_t H, int32_t dh, float* dqkv, float* delta, const tgmx_dropout_t* drop,
                                        tgmx_stream_t stream) {
  TGMX_REQUIRE(!drop || (drop->p >= 0.f && drop->p < 1.f), "mha_stream_backward: p must be in [0, 1)");
  TGMX_REQUIRE(stream_sizes_ok(B, T, H, dh, ldq, ldo), "mha_stream_backward: bad sizes B=%lld T=%d H=%d dh=%d", (long long)B, T, H, dh);
  if (!tgmx_mha_stream_supported(T, dh)) {
    set_error("mha_stream_backward: T=%d tokens x head dimension %d is outside the streaming envelope (%d < T <= %d, dh <= %d)", T, dh, kMhaMaxT,
              kStreamMaxT, kMhaMaxDh);
    return TGMX_E_UNSUPPORTED;
  }
  if (B == 0) return TGMX_OK;
  TGMX_REQUIRE(qkv && att && datt && lse && dqkv && delta && dqkv != qkv, "mha_stream_backward: null or aliased pointer");
  hipStream_t st = (hipStream_t)stream;
  const long long groups = (long long)B * T * H;
  hipLaunchKernelGGL(mha_stream_delta_kernel, dim3((unsigned)((groups + 15) / 16)), dim3(256), 0, st, att, datt, (long long)ldo, groups, T, H, dh, delta);
  TGMX_CHECK_LAUNCH("mha_stream_backward(delta)");
  const int NT = (dh + 15) / 16, nOB = (T + kStreamRows - 1) / kStreamRows;
  const float scale = 1.f / sqrtf((float)dh);
  const DropoutArgs da = make_dropout(drop);
  const dim3 grid((unsigned)(B * H * nOB));
#define CASE(N)                                                                                                                                    \
  do {                                                                                                                                             \
    hipLaunchKernelGGL((mha_stream_bwd_kernel<N, true>), grid, dim3(256), stream_bwd_lds(N, true), st, qkv, (long long)ldq, datt, (long long)ldo, lse, \
                       delta, T, H, dh, nOB, scale, dqkv, da);                                                                                     \
    hipLaunchKernelGGL((mha_stream_bwd_kernel<N, false>), grid, dim3(256), stream_bwd_lds(N, false), st, qkv, (long long)ldq, datt, (long long)ldo,   \
                       lse, delta, T, H, dh, nOB, scale, dqkv, da);                                                                                \
  } while (0)
  TGMX_STREAM_NT(NT, CASE)
#undef CASE
  TGMX_CHECK_LAUNCH("mha_stream_backward");
  return TGMX_OK;
}
