// CTAN training: the backward of tgmx_ctan_forward (csrc/ctan.hip) as one call, and its pieces.
//
//   tgmx_ctan_attend_backward   the target pass: one workgroup per target, the forward's walk twice (softmax state, then the per-edge terms)
//   tgmx_ctan_source_backward   the source pass: dk / dv gathered over the edges grouped by source -- no float atomics
//   tgmx_ctan_edge_attr_backward, tgmx_ctan_antisym_grad, tgmx_ctan_out_backward   the small pieces around them
//   tgmx_ctan_backward          the whole chain; GEMMs and reductions are the dense library's (csrc/dense.hip)
//
// What is recomputed: q | k | v | x A^T + bias of every iteration (the forward's batched GEMM on the saved x: the same call, the same bits)
// and the rows' softmax state (walk 1).  Every sum has a fixed order: ascending edge id inside a wave, waves merged in wave order.
#include <math.h>

#include "common.h"
#include "ctan_rows.h"
#include "edge_csr.h"
#include "lanes.h"

namespace tgmx {

struct CtanBwdArgs {
  CtanAttendArgs f;  // q, k, v, eproj, order, src, seg_lo, seg_hi, h4 (read only), U, C, scale, eps as the forward launch had them
  const float* gx;   // [U, C]
  float* d4;         // [U, 4C]: dq | dk | dv | dz
  float* alpha;      // [E]
  float* s;          // [E]
  int32_t* etgt;     // [E]
  float* d_eproj;    // [E, C] or null
  int accumulate;
};

// walk 2 over the n_here (<= 64) edges lanes 0 .. n_here - 1 hold: the forward's request discipline, two butterflies per edge
template <int V, bool VEC>
__device__ __forceinline__ void ctan_walk2_block(const CtanBwdArgs& b, const int tgt, const CtVec<V> q, const CtVec<V> dz, const float m, const float l,
                                                 const float delta, const int nv, const int col, const int my_e, const int my_j, const int n_here,
                                                 CtVec<V>& dq) {
  const CtanAttendArgs& a = b.f;
  const long long C = a.C;
  const float* __restrict__ kp = a.k + col;
  const float* __restrict__ vp = a.v + col;
  const float* __restrict__ ep = a.eproj + col;
  CtVec<V> kk[4], vv[4], ee[4], kn[4], vn[4], en[4];
  auto request = [&](int c0, CtVec<V> (&K)[4], CtVec<V> (&Vv)[4], CtVec<V> (&E)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int sl = c0 + s < n_here ? c0 + s : n_here - 1;
      const long long e = __builtin_amdgcn_readlane(my_e, sl), j = __builtin_amdgcn_readlane(my_j, sl);
      K[s] = ct_load<V, VEC>(kp + j * C, nv);
      Vv[s] = ct_load<V, VEC>(vp + j * C, nv);
      E[s] = ct_load<V, VEC>(ep + e * C, nv);
    }
  };
  request(0, kk, vv, ee);
  for (int c0 = 0; c0 < n_here; c0 += 4) {
    const bool more = c0 + 4 < n_here;
    if (more) request(c0 + 4, kn, vn, en);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (c0 + s < n_here) {  // wave-uniform
        const long long e = __builtin_amdgcn_readlane(my_e, c0 + s);
        float p = q.f[0] * (kk[s].f[0] + ee[s].f[0]);
        float da = dz.f[0] * (vv[s].f[0] + ee[s].f[0]);
#pragma unroll
        for (int u = 1; u < V; ++u) {
          p = __fmaf_rn(q.f[u], kk[s].f[u] + ee[s].f[u], p);
          da = __fmaf_rn(dz.f[u], vv[s].f[u] + ee[s].f[u], da);
        }
        p = lanes::butterfly_sum<1>(p);
        da = lanes::butterfly_sum<1>(da);
        const float al = expf(p * a.scale - m) / l;
        const float sv = a.scale * al * (da - delta);
#pragma unroll
        for (int u = 0; u < V; ++u) dq.f[u] = __fmaf_rn(sv, kk[s].f[u] + ee[s].f[u], dq.f[u]);
        if (b.d_eproj) {
          float* row = b.d_eproj + e * C + col;
          CtVec<V> de;
#pragma unroll
          for (int u = 0; u < V; ++u) de.f[u] = __fmaf_rn(sv, q.f[u], al * dz.f[u]);
          if (b.accumulate) {
            const CtVec<V> old = ct_load<V, VEC>(row, nv);
#pragma unroll
            for (int u = 0; u < V; ++u) de.f[u] += old.f[u];
          }
          ct_store<V, VEC>(row, nv, de);
        }
        if (lane_id() == 0) {
          b.alpha[e] = al;
          b.s[e] = sv;
          b.etgt[e] = tgt;
        }
      }
    }
    if (more) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        kk[s] = kn[s];
        vv[s] = vn[s];
        ee[s] = en[s];
      }
    }
  }
}

template <int V, bool VEC>
__global__ __launch_bounds__(256) void ctan_attend_backward_kernel(const CtanBwdArgs b) {
  const CtanAttendArgs& a = b.f;
  __shared__ float s_m[kCtanWaves], s_l[kCtanWaves];
  __shared__ float s_acc[kCtanWaves][kWave][V];
  __shared__ float s_dq[kCtanWaves][kWave][V];
  const long long i = blockIdx.x;
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const long long lo = a.seg_lo ? a.seg_lo[i] : 0, hi = a.seg_lo ? a.seg_hi[i] : 0;
  const long long n = hi > lo ? hi - lo : 0;
  const bool split = n > kCtanShort;  // (uniform over the workgroup: every barrier below is reached by all four waves or by none)
  if (!split && wave) return;
  const long long C = a.C;
  int nv = a.C - lane * V;
  nv = nv < 0 ? 0 : (nv > V ? V : nv);
  const int col = nv ? lane * V : 0;
  const CtVec<V> q = ct_load<V, VEC>(a.q + i * C + col, nv);
  // walk 1: the forward's, to the same (m, l, acc)
  CtanWalk<V> st;
  st.m = -__builtin_inff();
  st.l = 0.f;
#pragma unroll
  for (int u = 0; u < V; ++u) st.acc.f[u] = 0.f;
  int my_e = 0, my_j = 0;
  if (!split) {
    if (n) {
      if (lane < n) {
        my_e = (int)a.order[lo + lane];
        my_j = (int)a.src[my_e];
      }
      ctan_walk_block<V, VEC>(a, q, nv, col, my_e, my_j, (int)n, st);
    }
  } else {
    for (long long p0 = lo + wave; p0 < hi; p0 += (long long)kCtanWaves * kWave) {
      const long long my_p = p0 + (long long)kCtanWaves * lane;
      my_e = my_j = 0;
      if (my_p < hi) {
        my_e = (int)a.order[my_p];
        my_j = (int)a.src[my_e];
      }
      const long long left = (hi - p0 + kCtanWaves - 1) / kCtanWaves;
      ctan_walk_block<V, VEC>(a, q, nv, col, my_e, my_j, left < kWave ? (int)left : kWave, st);
    }
    if (lane == 0) {
      s_m[wave] = st.m;
      s_l[wave] = st.l;
    }
#pragma unroll
    for (int u = 0; u < V; ++u) s_acc[wave][lane][u] = st.acc.f[u];
    __syncthreads();
    // every wave merges (reads only): each needs the row's state for walk 2
    float M = s_m[0];
#pragma unroll
    for (int w2 = 1; w2 < kCtanWaves; ++w2) M = fmaxf(M, s_m[w2]);
    float L = 0.f;
    CtVec<V> A;
#pragma unroll
    for (int u = 0; u < V; ++u) A.f[u] = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < kCtanWaves; ++w2) {
      const float f = s_l[w2] > 0.f ? expf(s_m[w2] - M) : 0.f;
      L += s_l[w2] * f;
#pragma unroll
      for (int u = 0; u < V; ++u) A.f[u] += s_acc[w2][lane][u] * f;
    }
    st.m = M;
    st.l = L;
    st.acc = A;
  }
  // the epilogue's derivative: z = h4 + phi, dz = eps gx (1 - tanh^2 z), delta = dz . phi
  const CtVec<V> h = ct_load<V, VEC>(a.h4 + i * C + col, nv);
  const CtVec<V> g = ct_load<V, VEC>(b.gx + i * C + col, nv);
  CtVec<V> dz, dq;
  float delta = 0.f;
#pragma unroll
  for (int u = 0; u < V; ++u) {
    const float phi = n ? st.acc.f[u] / st.l : 0.f;
    const float tz = tanhf(h.f[u] + phi);
    dz.f[u] = a.eps * g.f[u] * (1.f - tz * tz);
    delta = __fmaf_rn(dz.f[u], phi, delta);
    dq.f[u] = 0.f;
  }
  delta = lanes::butterfly_sum<1>(delta);
  // walk 2
  if (!split) {
    if (n) ctan_walk2_block<V, VEC>(b, (int)i, q, dz, st.m, st.l, delta, nv, col, my_e, my_j, (int)n, dq);
  } else {
    for (long long p0 = lo + wave; p0 < hi; p0 += (long long)kCtanWaves * kWave) {
      const long long my_p = p0 + (long long)kCtanWaves * lane;
      my_e = my_j = 0;
      if (my_p < hi) {
        my_e = (int)a.order[my_p];
        my_j = (int)a.src[my_e];
      }
      const long long left = (hi - p0 + kCtanWaves - 1) / kCtanWaves;
      ctan_walk2_block<V, VEC>(b, (int)i, q, dz, st.m, st.l, delta, nv, col, my_e, my_j, left < kWave ? (int)left : kWave, dq);
    }
#pragma unroll
    for (int u = 0; u < V; ++u) s_dq[wave][lane][u] = dq.f[u];
    __syncthreads();
    if (wave) return;
#pragma unroll
    for (int u = 0; u < V; ++u) dq.f[u] = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < kCtanWaves; ++w2) {
#pragma unroll
      for (int u = 0; u < V; ++u) dq.f[u] += s_dq[w2][lane][u];
    }
  }
  float* row = b.d4 + i * 4 * C + col;
  ct_store<V, VEC>(row, nv, dq);
  ct_store<V, VEC>(row + 3 * C, nv, dz);
}

// ---- the source pass ------------------------------------------------------------------------------------------------------------------------
struct CtanSrcArgs {
  const float* q;          // [U, C]
  float* d4;               // [U, 4C]: reads dz (columns [3C, 4C)), writes dk, dv
  const int64_t* order;    // [E] edge ids stably sorted by source
  const int32_t* etgt;     // [E] target of every edge, in [0, U)
  const int64_t* seg_lo;   // [U]
  const int64_t* seg_hi;   // [U]
  const float* alpha;      // [E]
  const float* s;          // [E]
  long long U;
  int C;
};

// (etgt is the target pass's output; kept inside [0, U) here whatever it holds, so that no row address leaves d4)
__device__ __forceinline__ int ctan_row(int i, long long U) { return i < 0 ? 0 : (i >= U ? (int)U - 1 : i); }

// the n_here (<= 64) edges whose targets and scalars lanes 0 .. n_here - 1 hold, four at a time, the next four requested ahead
template <int V, bool VEC>
__device__ __forceinline__ void ctan_source_block(const CtanSrcArgs& a, const int nv, const int col, const int my_i, const float my_s, const float my_a,
                                                  const int n_here, CtVec<V>& dk, CtVec<V>& dv) {
  const long long C = a.C;
  const float* __restrict__ qp = a.q + col;
  const float* __restrict__ zp = a.d4 + 3 * C + col;
  CtVec<V> qq[4], zz[4], qn[4], zn[4];
  auto request = [&](int c0, CtVec<V> (&Q)[4], CtVec<V> (&Z)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int sl = c0 + s < n_here ? c0 + s : n_here - 1;
      const long long i = __builtin_amdgcn_readlane(my_i, sl);
      Q[s] = ct_load<V, VEC>(qp + i * C, nv);
      Z[s] = ct_load<V, VEC>(zp + i * 4 * C, nv);
    }
  };
  request(0, qq, zz);
  for (int c0 = 0; c0 < n_here; c0 += 4) {
    const bool more = c0 + 4 < n_here;
    if (more) request(c0 + 4, qn, zn);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (c0 + s < n_here) {  // wave-uniform
        const float sv = lanes::bcast(my_s, c0 + s), al = lanes::bcast(my_a, c0 + s);
#pragma unroll
        for (int u = 0; u < V; ++u) {
          dk.f[u] = __fmaf_rn(sv, qq[s].f[u], dk.f[u]);
          dv.f[u] = __fmaf_rn(al, zz[s].f[u], dv.f[u]);
        }
      }
    }
    if (more) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        qq[s] = qn[s];
        zz[s] = zn[s];
      }
    }
  }
}

template <int V, bool VEC>
__global__ __launch_bounds__(256) void ctan_source_backward_kernel(const CtanSrcArgs a) {
  __shared__ float s_dk[kCtanWaves][kWave][V];
  __shared__ float s_dv[kCtanWaves][kWave][V];
  const long long j = blockIdx.x;
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const long long lo = a.seg_lo ? a.seg_lo[j] : 0, hi = a.seg_lo ? a.seg_hi[j] : 0;
  const long long n = hi > lo ? hi - lo : 0;
  const bool split = n > kCtanShort;  // (uniform over the workgroup)
  if (!split && wave) return;
  const long long C = a.C;
  int nv = a.C - lane * V;
  nv = nv < 0 ? 0 : (nv > V ? V : nv);
  const int col = nv ? lane * V : 0;
  CtVec<V> dk, dv;
#pragma unroll
  for (int u = 0; u < V; ++u) dk.f[u] = dv.f[u] = 0.f;
  if (!split) {
    if (n) {
      int my_i = 0;
      float my_s = 0.f, my_a = 0.f;
      if (lane < n) {
        const long long e = a.order[lo + lane];
        my_i = ctan_row(a.etgt[e], a.U);
        my_s = a.s[e];
        my_a = a.alpha[e];
      }
      ctan_source_block<V, VEC>(a, nv, col, my_i, my_s, my_a, (int)n, dk, dv);
    }
  } else {
    for (long long p0 = lo + wave; p0 < hi; p0 += (long long)kCtanWaves * kWave) {
      const long long my_p = p0 + (long long)kCtanWaves * lane;
      int my_i = 0;
      float my_s = 0.f, my_a = 0.f;
      if (my_p < hi) {
        const long long e = a.order[my_p];
        my_i = ctan_row(a.etgt[e], a.U);
        my_s = a.s[e];
        my_a = a.alpha[e];
      }
      const long long left = (hi - p0 + kCtanWaves - 1) / kCtanWaves;
      ctan_source_block<V, VEC>(a, nv, col, my_i, my_s, my_a, left < kWave ? (int)left : kWave, dk, dv);
    }
#pragma unroll
    for (int u = 0; u < V; ++u) {
      s_dk[wave][lane][u] = dk.f[u];
      s_dv[wave][lane][u] = dv.f[u];
    }
    __syncthreads();
    if (wave) return;
#pragma unroll
    for (int u = 0; u < V; ++u) dk.f[u] = dv.f[u] = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < kCtanWaves; ++w2) {
#pragma unroll
      for (int u = 0; u < V; ++u) {
        dk.f[u] += s_dk[w2][lane][u];
        dv.f[u] += s_dv[w2][lane][u];
      }
    }
  }
  float* row = a.d4 + j * 4 * C + col;
  ct_store<V, VEC>(row + C, nv, dk);
  ct_store<V, VEC>(row + 2 * C, nv, dv);
}

// ---- the small pieces -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctan_out_backward_kernel(const float* __restrict__ g, long long ldg, const float* __restrict__ out, long long U,
                                                                int M, float* __restrict__ gx) {
  const long long total = U * M;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += step) {
    const long long r = p / M;
    const float o = out[p];
    gx[p] = g[r * ldg + (p - r * M)] * (1.f - o * o);
  }
}

// the layout twin of tconv_edge_attr_backward_kernel: the message first, rel as ctan_edge_attr_kernel computes it
__global__ __launch_bounds__(256) void ctan_edge_attr_backward_kernel(const int64_t* __restrict__ lu, const int64_t* __restrict__ src,
                                                                      const int64_t* __restrict__ t, const float* __restrict__ tw,
                                                                      const float* __restrict__ tb, const float* __restrict__ d_attr, long long ldd,
                                                                      int T, long long E, float mean, float std, float* __restrict__ part) {
  const long long total = E * T;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += step) {
    const long long e = x / T;
    const int c = (int)(x - e * T);
    long long d = lu[src[e]] - t[e];
    if (d < 0) d = -d;
    const float rel = ((float)d - mean) / std;
    const float gs = -sin_t2v(__fmaf_rn(rel, tw[c], tb[c])) * d_attr[e * ldd + c];
    part[e * 2LL * T + c] = gs * rel;
    part[e * 2LL * T + T + c] = gs;
  }
}

__global__ __launch_bounds__(256) void ctan_antisym_grad_kernel(const float* __restrict__ dA, int M, float* __restrict__ dW) {
  const int total = M * M;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += gridDim.x * blockDim.x) {
    const int r = p / M, c = p - r * M;
    dW[p] = dA[p] - dA[c * M + r];
  }
}

static unsigned ctan_blocks(long long total) {
  long long blocks = (total + 255) / 256;
  return (unsigned)(blocks > 16384 ? 16384 : (blocks < 1 ? 1 : blocks));
}

}  // namespace tgmx

using namespace tgmx;

extern "C" int tgmx_ctan_out_backward(const float* g, int64_t ldg, const float* out, int64_t U, int32_t M, float* gx, tgmx_stream_t stream) {
  TGMX_REQUIRE(U >= 0 && M > 0 && ldg >= M, "ctan_out_backward: bad sizes");
  if (U == 0) return TGMX_OK;
  TGMX_REQUIRE(g && out && gx, "ctan_out_backward: null pointer");
  hipLaunchKernelGGL(ctan_out_backward_kernel, dim3(ctan_blocks((long long)U * M)), dim3(256), 0, (hipStream_t)stream, g, (long long)ldg, out, (long long)U, M,
                     gx);
  TGMX_CHECK_LAUNCH("ctan_out_backward");
  return TGMX_OK;
}

extern "C" int tgmx_ctan_attend_backward(const float* q, const float* k, const float* v, const float* h4, const float* eproj, const int64_t* order,
                                         const int64_t* src, const int64_t* seg_lo, const int64_t* seg_hi, int64_t U, int32_t C, float scale,
                                         float epsilon, const float* gx, float* d4, float* alpha, float* s, int32_t* etgt, float* d_eproj,
                                         int32_t accumulate, tgmx_stream_t stream) {
  TGMX_REQUIRE(U >= 0 && U < (1ll << 31) && C > 0 && C <= kCtanMaxC, "ctan_attend_backward: bad sizes (C <= %d)", kCtanMaxC);
  if (U == 0) return TGMX_OK;
  TGMX_REQUIRE(q && h4 && gx && d4, "ctan_attend_backward: null pointer");
  TGMX_REQUIRE(!seg_lo || (k && v && eproj && order && src && seg_hi && alpha && s && etgt), "ctan_attend_backward: null pointer (edges)");
  CtanBwdArgs b{};
  b.f = CtanAttendArgs{q, k, v, eproj, order, src, seg_lo, seg_hi, const_cast<float*>(h4), nullptr, nullptr, U, C, scale, epsilon, 0, nullptr};
  b.gx = gx;
  b.d4 = d4;
  b.alpha = alpha;
  b.s = s;
  b.etgt = etgt;
  b.d_eproj = seg_lo ? d_eproj : nullptr;
  b.accumulate = accumulate ? 1 : 0;
  const int V = (C + kWave - 1) / kWave;
  const uintptr_t bits = (uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)eproj | (uintptr_t)h4 | (uintptr_t)gx | (uintptr_t)d4 | (uintptr_t)d_eproj;
  const dim3 grid((unsigned)U), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (V == 4 && C % 4 == 0 && (bits & 15) == 0) hipLaunchKernelGGL((ctan_attend_backward_kernel<4, true>), grid, block, 0, st, b);
  else if (V == 4) hipLaunchKernelGGL((ctan_attend_backward_kernel<4, false>), grid, block, 0, st, b);
  else if (V == 3) hipLaunchKernelGGL((ctan_attend_backward_kernel<3, false>), grid, block, 0, st, b);
  else if (V == 2 && C % 2 == 0 && (bits & 7) == 0) hipLaunchKernelGGL((ctan_attend_backward_kernel<2, true>), grid, block, 0, st, b);
  else if (V == 2) hipLaunchKernelGGL((ctan_attend_backward_kernel<2, false>), grid, block, 0, st, b);
  else hipLaunchKernelGGL((ctan_attend_backward_kernel<1, false>), grid, block, 0, st, b);
  TGMX_CHECK_LAUNCH("ctan_attend_backward");
  return TGMX_OK;
}

extern "C" int tgmx_ctan_source_backward(const float* q, float* d4, const int64_t* order_s, const int32_t* etgt, const int64_t* sseg_lo,
                                         const int64_t* sseg_hi, const float* alpha, const float* s, int64_t U, int32_t C, tgmx_stream_t stream) {
  TGMX_REQUIRE(U >= 0 && U < (1ll << 31) && C > 0 && C <= kCtanMaxC, "ctan_source_backward: bad sizes (C <= %d)", kCtanMaxC);
  if (U == 0) return TGMX_OK;
  TGMX_REQUIRE(d4 && (!sseg_lo || (q && order_s && etgt && sseg_hi && alpha && s)), "ctan_source_backward: null pointer");
  const CtanSrcArgs a{q, d4, order_s, etgt, sseg_lo, sseg_hi, alpha, s, U, C};
  const int V = (C + kWave - 1) / kWave;
  const uintptr_t bits = (uintptr_t)q | (uintptr_t)d4;
  const dim3 grid((unsigned)U), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (V == 4 && C % 4 == 0 && (bits & 15) == 0) hipLaunchKernelGGL((ctan_source_backward_kernel<4, true>), grid, block, 0, st, a);
  else if (V == 4) hipLaunchKernelGGL((ctan_source_backward_kernel<4, false>), grid, block, 0, st, a);
  else if (V == 3) hipLaunchKernelGGL((ctan_source_backward_kernel<3, false>), grid, block, 0, st, a);
  else if (V == 2 && C % 2 == 0 && (bits & 7) == 0) hipLaunchKernelGGL((ctan_source_backward_kernel<2, true>), grid, block, 0, st, a);
  else if (V == 2) hipLaunchKernelGGL((ctan_source_backward_kernel<2, false>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((ctan_source_backward_kernel<1, false>), grid, block, 0, st, a);
  TGMX_CHECK_LAUNCH("ctan_source_backward");
  return TGMX_OK;
}

extern "C" int tgmx_ctan_edge_attr_backward(const int64_t* last_update, const int64_t* src, const int64_t* t, const float* tw, const float* tb,
                                            const float* d_attr, int64_t ldd, int32_t T, int64_t E, float mean, float std, float* part,
                                            tgmx_stream_t stream) {
  TGMX_REQUIRE(T > 0 && E >= 0 && ldd >= T, "ctan_edge_attr_backward: bad sizes");
  if (E == 0) return TGMX_OK;
  TGMX_REQUIRE(last_update && src && t && tw && tb && d_attr && part, "ctan_edge_attr_backward: null pointer");
  hipLaunchKernelGGL(ctan_edge_attr_backward_kernel, dim3(ctan_blocks((long long)E * T)), dim3(256), 0, (hipStream_t)stream, last_update, src, t, tw, tb,
                     d_attr, (long long)ldd, T, (long long)E, mean, std, part);
  TGMX_CHECK_LAUNCH("ctan_edge_attr_backward");
  return TGMX_OK;
}

extern "C" int tgmx_ctan_antisym_grad(const float* dA, int32_t M, float* dW, tgmx_stream_t stream) {
  TGMX_REQUIRE(M > 0 && M <= 16384, "ctan_antisym_grad: bad sizes");
  TGMX_REQUIRE(dA && dW && dA != dW, "ctan_antisym_grad: null or aliased pointer");
  hipLaunchKernelGGL(ctan_antisym_grad_kernel, dim3(ctan_blocks((long long)M * M)), dim3(256), 0, (hipStream_t)stream, dA, M, dW);
  TGMX_CHECK_LAUNCH("ctan_antisym_grad");
  return TGMX_OK;
}

// ---- the whole backward as one call ---------------------------------------------------------------------------------------------------------
static int ctan_bwd_check(const tgmx_ctan_bwd_t* a, const char* what) {
  TGMX_REQUIRE(a, "%s: null argument block", what);
  TGMX_REQUIRE(a->U >= 0 && a->U < (1ll << 31) && a->E >= 0 && a->E < (1ll << 31) && a->M > 0 && a->M <= kCtanMaxC && a->in_ch > 0 && a->T > 0 &&
                   a->D >= 0 && a->num_iters >= 0,
               "%s: bad sizes (M <= %d)", what, kCtanMaxC);
  TGMX_REQUIRE(a->ldg >= a->M || a->U == 0, "%s: leading dimension of the upstream gradient", what);
  TGMX_REQUIRE(!a->d_W || a->d_W4, "%s: d_W needs d_W4", what);
  return TGMX_OK;
}

static int ctan_zero(float* p, size_t n, hipStream_t st) {
  if (p && n && hipMemsetAsync(p, 0, n * sizeof(float), st) != hipSuccess) {
    set_error("ctan_backward: hipMemsetAsync failed");
    return TGMX_E_LAUNCH;
  }
  return TGMX_OK;
}

// dry: lay the workspace out only (*need = its size), launch nothing
static int ctan_backward_pass(const tgmx_ctan_bwd_t* a, bool dry, size_t* need, tgmx_stream_t stream) {
  const int64_t U = a->U, E = a->E;
  const int M = a->M, Wd = a->D + a->T, T = a->T, n_it = a->num_iters;
  const bool walk = n_it > 0 && E > 0;                        // the attention passes run
  const bool want_e = walk && (a->d_Wedge || a->d_time);      // somebody reads d_eproj
  const bool want_x0 = a->d_Wx || a->d_bx || a->d_node_x;     // somebody reads the gradient at enc_x's output
  hipStream_t st = (hipStream_t)stream;
  WorkspaceCarver ws(dry ? nullptr : a->workspace);
  int rc;
  const size_t UM = (size_t)U * M, e1 = E > 0 ? (size_t)E : 1;
  float* gx = ws.take<float>(UM);
  float* gx2 = ws.take<float>(UM);
  float* qkvs = ws.take<float>(4 * UM);
  float* d4 = ws.take<float>(4 * UM);
  float* alpha = ws.take<float>(e1);
  float* sc = ws.take<float>(e1);
  int32_t* etgt = ws.take<int32_t>(e1);
  int64_t* order_s = ws.take<int64_t>(e1);
  int64_t* sseg_lo = ws.take<int64_t>((size_t)U);
  int64_t* sseg_hi = ws.take<int64_t>((size_t)U);
  int32_t* status = ws.take<int32_t>(1);
  const size_t sort_bytes = walk ? tgmx_segment_sort_workspace_bytes(E) : 0;
  char* sort_ws = ws.take<char>(sort_bytes);
  float* d_eproj = ws.take<float>(want_e ? (size_t)E * M : 0);
  float* d_attr = ws.take<float>(want_e && a->d_time ? (size_t)E * T : 0);
  float* part = ws.take<float>(want_e && a->d_time ? (size_t)E * 2 * T : 0);
  size_t tn_bytes = tgmx_sgemm_tn_workspace_bytes(U, M, M, 4);
  const size_t tn_x = tgmx_sgemm_tn_workspace_bytes(U, M, a->in_ch, 1), tn_e = E ? tgmx_sgemm_tn_workspace_bytes(E, M, Wd, 1) : 0;
  tn_bytes = tn_bytes > tn_x ? tn_bytes : tn_x;
  tn_bytes = tn_bytes > tn_e ? tn_bytes : tn_e;
  float* tn_ws = ws.take<float>(tn_bytes / sizeof(float) + 1);
  const int widest = 4 * M > 2 * T ? 4 * M : 2 * T;
  float* cs_ws = ws.take<float>((size_t)256 * widest);
  *need = ws.total();
  if (dry) return TGMX_OK;

  // 1. the final tanh
  if ((rc = tgmx_ctan_out_backward(a->g, a->ldg, a->out, U, M, gx, stream))) return rc;
  // 2. the iterations, last first
  if (walk) {
    if (hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess) {
      set_error("ctan_backward: hipMemsetAsync failed");
      return TGMX_E_LAUNCH;
    }
    if ((rc = tgmx_segment_sort(a->src_ok, E, (int32_t)U, order_s, sseg_lo, sseg_hi, sort_ws, sort_bytes, status, stream))) return rc;
  }
  const float scale = 1.0f / sqrtf((float)M);
  const float* h4 = qkvs + 3 * UM;
  for (int it = n_it - 1; it >= 0; --it) {
    const float* x = a->x_save + (size_t)it * UM;
    const bool first = it == n_it - 1;
    if ((rc = tgmx_sgemm_nt(x, M, a->W4, M, qkvs, M, U, M, M, a->b4, 0, 4, 0, (long long)M * M, U * M, stream))) return rc;
    if ((rc = tgmx_ctan_attend_backward(qkvs, qkvs + UM, qkvs + 2 * UM, h4, a->eproj, a->order, a->src_ok, E ? a->seg_lo : nullptr, a->seg_hi, U, M, scale,
                                  a->epsilon, gx, d4, alpha, sc, etgt, want_e ? d_eproj : nullptr, first ? 0 : 1, stream))) return rc;
    if ((rc = tgmx_ctan_source_backward(qkvs, d4, order_s, etgt, E ? sseg_lo : nullptr, sseg_hi, alpha, sc, U, M, stream))) return rc;
    if (a->d_W4 && (rc = tgmx_sgemm_tn(d4, 4 * M, x, M, a->d_W4, M, U, M, M, 4, M, 0, (long long)M * M, first ? 0 : 1, tn_ws, stream))) return rc;
    if (a->d_b4 && (rc = tgmx_colsum(d4, 4 * M, U, 4 * M, a->d_b4, first ? 0 : 1, cs_ws, stream))) return rc;
    if (it > 0 || want_x0) {
      if ((rc = tgmx_sgemm_nt_ep(d4, 4 * M, a->W4T, 4 * M, gx2, M, U, M, 4 * M, nullptr, 0, gx, M, stream))) return rc;
      float* tmp = gx;
      gx = gx2;
      gx2 = tmp;
    }
  }
  // 3. what lies around the loop
  if (n_it == 0) {
    if ((rc = ctan_zero(a->d_W4, (size_t)4 * M * M, st)) || (rc = ctan_zero(a->d_b4, (size_t)4 * M, st))) return rc;
  }
  if (a->d_W && (rc = tgmx_ctan_antisym_grad(a->d_W4 + (size_t)3 * M * M, M, a->d_W, stream))) return rc;
  if (a->d_Wx && (rc = tgmx_sgemm_tn(gx, M, a->node_x, a->in_ch, a->d_Wx, a->in_ch, U, M, a->in_ch, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
  if (a->d_bx && (rc = tgmx_colsum(gx, M, U, M, a->d_bx, 0, cs_ws, stream))) return rc;
  if (a->d_node_x && (rc = tgmx_sgemm_nt(gx, M, a->WxT, M, a->d_node_x, a->in_ch, U, a->in_ch, M, nullptr, 0, 1, 0, 0, 0, stream))) return rc;
  if (!want_e) {
    if ((rc = ctan_zero(a->d_Wedge, (size_t)M * Wd, st)) || (rc = ctan_zero(a->d_time, (size_t)2 * T, st))) return rc;
  } else {
    if (a->d_Wedge && (rc = tgmx_sgemm_tn(d_eproj, M, a->edge_attr, Wd, a->d_Wedge, Wd, E, M, Wd, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
    if (a->d_time) {
      if ((rc = tgmx_sgemm_nt(d_eproj, M, a->WeT, M, d_attr, T, E, T, M, nullptr, 0, 1, 0, 0, 0, stream))) return rc;
      if ((rc = tgmx_ctan_edge_attr_backward(a->last_update, a->src_ok, a->t, a->tw, a->tb, d_attr, T, T, E, a->mean_delta_t, a->std_delta_t, part, stream))) return rc;
      if ((rc = tgmx_colsum(part, 2 * T, E, 2 * T, a->d_time, 0, cs_ws, stream))) return rc;
    }
  }
  return TGMX_OK;
}

extern "C" size_t tgmx_ctan_backward_workspace_bytes(const tgmx_ctan_bwd_t* a) {
  size_t need = 0;
  if (ctan_bwd_check(a, "ctan_backward_workspace_bytes") != TGMX_OK) return 0;
  return ctan_backward_pass(a, true, &need, nullptr) == TGMX_OK ? need : 0;
}

extern "C" int tgmx_ctan_backward(const tgmx_ctan_bwd_t* a, tgmx_stream_t stream) {
  int rc;
  if ((rc = ctan_bwd_check(a, "ctan_backward"))) return rc;
  if (a->U == 0) return TGMX_OK;
  const bool walk = a->num_iters > 0 && a->E > 0;
  TGMX_REQUIRE(a->g && a->out && a->x_save, "ctan_backward: the upstream gradient or the forward's saved buffers are missing");
  TGMX_REQUIRE(a->num_iters == 0 || (a->W4 && a->b4 && a->W4T), "ctan_backward: the stacked weights are missing");
  TGMX_REQUIRE(!walk || (a->eproj && a->src_ok && a->order && a->seg_lo && a->seg_hi), "ctan_backward: the forward's edge buffers are missing");
  TGMX_REQUIRE(!a->d_Wx || a->node_x, "ctan_backward: d_Wx needs node_x");
  TGMX_REQUIRE(!a->d_node_x || a->WxT, "ctan_backward: d_node_x needs the transposed enc_x weight");
  TGMX_REQUIRE(!(walk && a->d_Wedge) || a->edge_attr, "ctan_backward: d_Wedge needs edge_attr");
  TGMX_REQUIRE(!(walk && a->d_time) || (a->WeT && a->last_update && a->t && a->tw && a->tb), "ctan_backward: d_time needs the time encoder's inputs");
  size_t need = 0;
  if ((rc = ctan_backward_pass(a, true, &need, nullptr))) return rc;
  TGMX_REQUIRE(a->workspace && a->workspace_bytes >= need, "ctan_backward: workspace too small (%zu bytes, %zu needed)", a->workspace_bytes, need);
  return ctan_backward_pass(a, false, &need, stream);
}
