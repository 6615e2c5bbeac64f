// TransformerConv training for wide heads: a deterministic attention backward (target pass + source pass, no float atomics) and the whole
// layer's backward as one call.  The form is CTAN's (csrc/ctan_bwd.hip); what differs is the layer: several heads, dropout on the
// coefficients, a skip projection.
//
//   tgmx_tconv_train_supported        the envelope: C <= 256, H <= 8, H C <= 512
//   tgmx_tconv_attend_backward_det    target pass -> edges grouped by source (tgmx_segment_sort) -> source pass
//   tgmx_tconv_backward               the layer: the two groupings, the attention backward, then the dense library's GEMMs and reductions
//
// Lane layout (both kernels).  The H C columns of a row are dealt to the 64 lanes head by head: with Hp = H rounded up to a power of two a
// head owns G = 64 / Hp consecutive lanes, lane (h, cl) = (lane / G, lane % G) owns the V columns h C + cl V .. + V - 1 of every row it
// touches, V = the smallest of 2, 4, 8, 16 with G V >= C.  No vector straddles a head, so a head's dot product is a butterfly over the
// xor offsets 1 .. G / 2 inside its lane group and every lane of a group ends up with the head's score: all heads are scored in the SAME
// walk and every k, v, eproj row is read once per walk.  A lane's piece is moved as 16-, 8- or 4-byte accesses (VW = 4, 2, 1 floats): the
// widest that C, the leading dimensions and the pointers allow; nv = how many of the lane's V columns exist (C = 86: the last lane of a
// head holds 2 of 4, the lanes behind it none).
//
// Rows in flight: an edge block is B = min(4, 16 / V) edges; the 3 B row pieces of the NEXT block are requested before the current block
// is scored (edge ids and sources come out of lanes by v_readlane).
//
// Order of every sum: ascending position inside a wave, waves merged in wave order, columns of a lane in ascending order, then the
// butterfly.  Two launches give the same bits.
//
// Rounding chain (oracle/tgn_bwd_ref.py: attend_chain counts 2C + 3L + 16 + outdeg + 8 for the one-wave kernel).  Here a score is V fmas and
// log2 G butterfly adds (<= C), a wave's l / acc chain is at most max(L, 16) / 4 + 4 links with the merge, delta is V fmas and the butterfly,
// dq is one fma per edge of the wave plus 4 merge adds, dk / dv one fma per outgoing edge of the wave plus 4: every chain is no longer than
// the one counted there, so that count bounds these kernels too.
#include <math.h>

#include "common.h"
#include "edge_csr.h"
#include "lanes.h"

namespace tgmx {

constexpr int kTvShort = 16;  // segments of up to this many edges run on one wave
constexpr int kTvWaves = 4;
constexpr int kTvMaxH = 8, kTvMaxC = 256, kTvMaxHC = 512;

static bool tv_supported(int H, int C) { return H >= 1 && H <= kTvMaxH && C >= 1 && C <= kTvMaxC && H * C <= kTvMaxHC; }

struct TvLayout {
  int G, V;
};
static TvLayout tv_layout(int H, int C) {
  int Hp = 1;
  while (Hp < H) Hp <<= 1;
  const int G = kWave / Hp;
  int V = 2;
  while (G * V < C) V <<= 1;  // (inside the envelope: V <= 16)
  return {G, V};
}

template <int V>
struct TvVec {
  float f[V];
};
template <int V>
constexpr int tv_block() {
  return V <= 4 ? 4 : 16 / V;
}

// the lane's piece of a row: p points at its first column, nv of its V columns exist (a multiple of VW)
template <int V, int VW>
__device__ __forceinline__ TvVec<V> tv_load(const float* __restrict__ p, const int nv) {
  TvVec<V> r;
  if constexpr (VW == 4) {
#pragma unroll
    for (int c = 0; c < V; c += 4) {
      const float4 x = c < nv ? *reinterpret_cast<const float4*>(p + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      r.f[c] = x.x; r.f[c + 1] = x.y; r.f[c + 2] = x.z; r.f[c + 3] = x.w;
    }
  } else if constexpr (VW == 2) {
#pragma unroll
    for (int c = 0; c < V; c += 2) {
      const float2 x = c < nv ? *reinterpret_cast<const float2*>(p + c) : make_float2(0.f, 0.f);
      r.f[c] = x.x; r.f[c + 1] = x.y;
    }
  } else {
#pragma unroll
    for (int u = 0; u < V; ++u) r.f[u] = u < nv ? p[u] : 0.f;
  }
  return r;
}
template <int V, int VW>
__device__ __forceinline__ void tv_store(float* __restrict__ p, const int nv, const TvVec<V>& r) {
  if constexpr (VW == 4) {
#pragma unroll
    for (int c = 0; c < V; c += 4)
      if (c < nv) *reinterpret_cast<float4*>(p + c) = make_float4(r.f[c], r.f[c + 1], r.f[c + 2], r.f[c + 3]);
  } else if constexpr (VW == 2) {
#pragma unroll
    for (int c = 0; c < V; c += 2)
      if (c < nv) *reinterpret_cast<float2*>(p + c) = make_float2(r.f[c], r.f[c + 1]);
  } else {
#pragma unroll
    for (int u = 0; u < V; ++u)
      if (u < nv) p[u] = r.f[u];
  }
}
template <int V>
__device__ __forceinline__ TvVec<V> tv_zero() {
  TvVec<V> r;
#pragma unroll
  for (int u = 0; u < V; ++u) r.f[u] = 0.f;
  return r;
}

// sum over the G lanes of a head (G = 8, 16, 32, 64, wave-uniform): xor 1, 2, 4, then 8, 16, 32 as far as the group reaches
__device__ __forceinline__ float tv_group_sum(float v, const int G) {
  v += lanes::lane_xor<1>(v);
  v += lanes::lane_xor<2>(v);
  v += lanes::lane_xor<4>(v);
  if (G > 8) v += lanes::lane_xor<8>(v);
  if (G > 16) v += lanes::lane_xor<16>(v);
  if (G > 32) v += lanes::lane_xor<32>(v);
  return v;
}

// where a lane sits: its head (clamped for the lane groups behind the last head, which own nothing), its first column, its column count
struct TvLane {
  int h, cl, nv, col;
  bool head_on;
};
template <int V>
__device__ __forceinline__ TvLane tv_lane(const int lane, const int H, const int C, const int G) {
  TvLane L;
  const int hr = lane / G;  // (G is a power of two)
  L.cl = lane & (G - 1);
  L.head_on = hr < H;
  L.h = L.head_on ? hr : H - 1;
  int nv = L.head_on ? C - L.cl * V : 0;
  L.nv = nv < 0 ? 0 : (nv > V ? V : nv);
  L.col = L.nv ? L.h * C + L.cl * V : 0;
  return L;
}

// (edge ids, sources and targets are kept inside their ranges whatever the index tensors hold, so that no row address leaves its tensor)
__device__ __forceinline__ int tv_clamp(long long i, long long n) { return (int)(i < 0 ? 0 : (i >= n ? n - 1 : i)); }

// ---- the target pass --------------------------------------------------------------------------------------------------------------------
struct TvArgs {
  const float *q, *k, *v;  // [U, H*C] each, rows ldq apart
  long long ldq;
  const float* eproj;      // [E, H*C], original edge order
  const int64_t* order;    // [E] edge ids grouped by target, ascending inside a segment
  const int64_t* src;      // [E] source of every edge
  const int64_t* seg_lo;   // [U] (null: no edges)
  const int64_t* seg_hi;   // [U]
  const float* dout;       // [U, H*C], rows ldg apart
  long long ldg;
  float* dq;               // [U, H*C], rows ldd apart
  float* gcopy;            // null, or [U, H*C] rows ldd apart: receives dout (the layer's d4 = dq | dk | dv | dout)
  long long ldd;
  float* de;               // [E, H*C]
  float* sc;               // [E, H, 2]: ds, ad = alpha mk
  int32_t* etgt;           // [E]
  int32_t* status_zero;    // the source grouping's status word, cleared here (one launch ahead of the sort that raises it)
  long long U, E;
  int H, C, G;
  float scale;
  DropoutArgs drop;        // element e * H + h, as the forward
};

// walk 1 over the n_here (<= 64) edges whose ids / sources lanes 0 .. n_here - 1 hold: the forward's online softmax, every head at once
template <int V, int VW>
__device__ __forceinline__ void tv_walk1(const TvArgs& a, const TvVec<V>& q, const TvLane& L, const int my_e, const int my_j, const int n_here,
                                         float& m_io, float& l_io, TvVec<V>& acc_io) {
  constexpr int B = tv_block<V>();
  const long long HC = (long long)a.H * a.C;
  const float* __restrict__ kp = a.k + L.col;
  const float* __restrict__ vp = a.v + L.col;
  const float* __restrict__ ep = a.eproj + L.col;
  TvVec<V> kk[B], vv[B], ee[B], kn[B], vn[B], en[B];
  auto request = [&](int c0, TvVec<V> (&K)[B], TvVec<V> (&Vv)[B], TvVec<V> (&E)[B]) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < B; ++s) {
      const int sl = c0 + s < n_here ? c0 + s : n_here - 1;  // (clamped: a position past the block re-reads its last edge, not used below)
      const long long e = __builtin_amdgcn_readlane(my_e, sl), j = __builtin_amdgcn_readlane(my_j, sl);
      K[s] = tv_load<V, VW>(kp + j * a.ldq, L.nv);
      Vv[s] = tv_load<V, VW>(vp + j * a.ldq, L.nv);
      E[s] = tv_load<V, VW>(ep + e * HC, L.nv);
    }
  };
  request(0, kk, vv, ee);
  float m = m_io, l = l_io;
  TvVec<V> acc = acc_io;
  for (int c0 = 0; c0 < n_here; c0 += B) {
    const bool more = c0 + B < n_here;
    if (more) request(c0 + B, kn, vn, en);
#pragma unroll
    for (int s = 0; s < B; ++s) {
      if (c0 + s < n_here) {  // wave-uniform
        float p = q.f[0] * (kk[s].f[0] + ee[s].f[0]);
#pragma unroll
        for (int u = 1; u < V; ++u) p = __fmaf_rn(q.f[u], kk[s].f[u] + ee[s].f[u], p);
        p = tv_group_sum(p, a.G);
        const float sc = p * a.scale;
        const float mn = sc > m ? sc : m;
        const float corr = expf(m - mn), w = expf(sc - mn);
        const long long e = __builtin_amdgcn_readlane(my_e, c0 + s);
        const float wd = w * dropout_scale(a.drop, (unsigned long long)e * a.H + L.h);
#pragma unroll
        for (int u = 0; u < V; ++u) acc.f[u] = acc.f[u] * corr + wd * (vv[s].f[u] + ee[s].f[u]);
        l = l * corr + w;
        m = mn;
      }
    }
    if (more) {
#pragma unroll
      for (int s = 0; s < B; ++s) {
        kk[s] = kn[s];
        vv[s] = vn[s];
        ee[s] = en[s];
      }
    }
  }
  m_io = m;
  l_io = l;
  acc_io = acc;
}

// walk 2: per edge alpha, ds, ad; the de row, the scalars and the target for the source pass; dq in registers
template <int V, int VW>
__device__ __forceinline__ void tv_walk2(const TvArgs& a, const int tgt, const TvVec<V>& q, const TvVec<V>& g, const float m, const float l,
                                         const float delta, const TvLane& L, const int my_e, const int my_j, const int n_here, TvVec<V>& dq) {
  constexpr int B = tv_block<V>();
  const long long HC = (long long)a.H * a.C;
  const float* __restrict__ kp = a.k + L.col;
  const float* __restrict__ vp = a.v + L.col;
  const float* __restrict__ ep = a.eproj + L.col;
  TvVec<V> kk[B], vv[B], ee[B], kn[B], vn[B], en[B];
  auto request = [&](int c0, TvVec<V> (&K)[B], TvVec<V> (&Vv)[B], TvVec<V> (&E)[B]) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < B; ++s) {
      const int sl = c0 + s < n_here ? c0 + s : n_here - 1;
      const long long e = __builtin_amdgcn_readlane(my_e, sl), j = __builtin_amdgcn_readlane(my_j, sl);
      K[s] = tv_load<V, VW>(kp + j * a.ldq, L.nv);
      Vv[s] = tv_load<V, VW>(vp + j * a.ldq, L.nv);
      E[s] = tv_load<V, VW>(ep + e * HC, L.nv);
    }
  };
  request(0, kk, vv, ee);
  for (int c0 = 0; c0 < n_here; c0 += B) {
    const bool more = c0 + B < n_here;
    if (more) request(c0 + B, kn, vn, en);
#pragma unroll
    for (int s = 0; s < B; ++s) {
      if (c0 + s < n_here) {  // wave-uniform
        const long long e = __builtin_amdgcn_readlane(my_e, c0 + s);
        float p = q.f[0] * (kk[s].f[0] + ee[s].f[0]);
        float dal = g.f[0] * (vv[s].f[0] + ee[s].f[0]);
#pragma unroll
        for (int u = 1; u < V; ++u) {
          p = __fmaf_rn(q.f[u], kk[s].f[u] + ee[s].f[u], p);
          dal = __fmaf_rn(g.f[u], vv[s].f[u] + ee[s].f[u], dal);
        }
        p = tv_group_sum(p, a.G);
        dal = tv_group_sum(dal, a.G);
        const float al = expf(p * a.scale - m) / l;
        const float mk = dropout_scale(a.drop, (unsigned long long)e * a.H + L.h);
        const float ds = al * (dal * mk - delta) * a.scale;  // softmax backward on the pre-dropout coefficients
        const float ad = al * mk;                            // the coefficient the value actually got
        TvVec<V> de;
#pragma unroll
        for (int u = 0; u < V; ++u) {
          dq.f[u] = __fmaf_rn(ds, kk[s].f[u] + ee[s].f[u], dq.f[u]);
          de.f[u] = __fmaf_rn(ds, q.f[u], ad * g.f[u]);
        }
        tv_store<V, VW>(a.de + e * HC + L.col, L.nv, de);
        if (L.cl == 0 && L.head_on) *reinterpret_cast<float2*>(a.sc + (e * a.H + L.h) * 2) = make_float2(ds, ad);
        if (lane_id() == 0) a.etgt[e] = tgt;
      }
    }
    if (more) {
#pragma unroll
      for (int s = 0; s < B; ++s) {
        kk[s] = kn[s];
        vv[s] = vn[s];
        ee[s] = en[s];
      }
    }
  }
}

template <int V, int VW>
__global__ __launch_bounds__(256) void tconv_target_backward_kernel(const TvArgs a) {
  __shared__ float s_m[kTvWaves][kTvMaxH], s_l[kTvWaves][kTvMaxH];
  __shared__ float s_vec[kTvWaves][kWave][V];  // the waves' acc partials, then (behind a barrier) their dq partials
  const long long i = blockIdx.x;
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  if (a.status_zero && i == 0 && threadIdx.x == 0) *a.status_zero = 0;
  const long long lo = a.seg_lo ? a.seg_lo[i] : 0, hi = a.seg_lo ? a.seg_hi[i] : 0;
  const long long n = hi > lo ? hi - lo : 0;
  const bool split = n > kTvShort;  // (uniform over the workgroup: every barrier below is reached by all four waves or by none)
  if (!split && wave) return;
  const TvLane L = tv_lane<V>(lane, a.H, a.C, a.G);
  const TvVec<V> q = tv_load<V, VW>(a.q + i * a.ldq + L.col, L.nv);
  const TvVec<V> g = tv_load<V, VW>(a.dout + i * a.ldg + L.col, L.nv);
  if (wave == 0 && a.gcopy) tv_store<V, VW>(a.gcopy + i * a.ldd + L.col, L.nv, g);
  TvVec<V> dq = tv_zero<V>();
  if (n == 0) {  // no incoming edge: only the skip term reached the output
    tv_store<V, VW>(a.dq + i * a.ldd + L.col, L.nv, dq);
    return;
  }
  // walk 1: the forward's, to the same (m, l, acc) per head
  float m = -__builtin_inff(), l = 0.f;
  TvVec<V> acc = tv_zero<V>();
  int my_e = 0, my_j = 0;
  if (!split) {
    if (lane < n) {
      my_e = tv_clamp(a.order[lo + lane], a.E);
      my_j = tv_clamp(a.src[my_e], a.U);
    }
    tv_walk1<V, VW>(a, q, L, my_e, my_j, (int)n, m, l, acc);
  } else {
    for (long long p0 = lo + wave; p0 < hi; p0 += (long long)kTvWaves * kWave) {
      const long long my_p = p0 + (long long)kTvWaves * lane;
      my_e = my_j = 0;
      if (my_p < hi) {
        my_e = tv_clamp(a.order[my_p], a.E);
        my_j = tv_clamp(a.src[my_e], a.U);
      }
      const long long left = (hi - p0 + kTvWaves - 1) / kTvWaves;
      tv_walk1<V, VW>(a, q, L, my_e, my_j, left < kWave ? (int)left : kWave, m, l, acc);
    }
    if (L.cl == 0 && L.head_on) {
      s_m[wave][L.h] = m;
      s_l[wave][L.h] = l;
    }
#pragma unroll
    for (int u = 0; u < V; ++u) s_vec[wave][lane][u] = acc.f[u];
    __syncthreads();
    // every wave merges (reads only): each needs the heads' state for walk 2
    float M = s_m[0][L.h];
#pragma unroll
    for (int w2 = 1; w2 < kTvWaves; ++w2) M = fmaxf(M, s_m[w2][L.h]);
    float Lsum = 0.f;
    TvVec<V> A = tv_zero<V>();
#pragma unroll
    for (int w2 = 0; w2 < kTvWaves; ++w2) {
      const float f = s_l[w2][L.h] > 0.f ? expf(s_m[w2][L.h] - M) : 0.f;  // a wave without edges has m = -inf, l = 0
      Lsum += s_l[w2][L.h] * f;
#pragma unroll
      for (int u = 0; u < V; ++u) A.f[u] += s_vec[w2][lane][u] * f;
    }
    m = M;
    l = Lsum;
    acc = A;
    __syncthreads();  // s_vec is free for the dq partials
  }
  // delta = sum_p alpha_p mk_p (dout . val_p) = dout . (the dropped attention output), per head
  float delta = 0.f;
#pragma unroll
  for (int u = 0; u < V; ++u) delta = __fmaf_rn(g.f[u], acc.f[u] / l, delta);
  delta = tv_group_sum(delta, a.G);
  // walk 2
  if (!split) {
    tv_walk2<V, VW>(a, (int)i, q, g, m, l, delta, L, my_e, my_j, (int)n, dq);
  } else {
    for (long long p0 = lo + wave; p0 < hi; p0 += (long long)kTvWaves * kWave) {
      const long long my_p = p0 + (long long)kTvWaves * lane;
      my_e = my_j = 0;
      if (my_p < hi) {
        my_e = tv_clamp(a.order[my_p], a.E);
        my_j = tv_clamp(a.src[my_e], a.U);
      }
      const long long left = (hi - p0 + kTvWaves - 1) / kTvWaves;
      tv_walk2<V, VW>(a, (int)i, q, g, m, l, delta, L, my_e, my_j, left < kWave ? (int)left : kWave, dq);
    }
#pragma unroll
    for (int u = 0; u < V; ++u) s_vec[wave][lane][u] = dq.f[u];
    __syncthreads();
    if (wave) return;
    dq = tv_zero<V>();
#pragma unroll
    for (int w2 = 0; w2 < kTvWaves; ++w2) {
#pragma unroll
      for (int u = 0; u < V; ++u) dq.f[u] += s_vec[w2][lane][u];
    }
  }
  tv_store<V, VW>(a.dq + i * a.ldd + L.col, L.nv, dq);
}

// ---- the source pass --------------------------------------------------------------------------------------------------------------------
struct TvSrcArgs {
  const float* q;          // [U, H*C], rows ldq apart
  long long ldq;
  const float* dout;       // [U, H*C], rows ldg apart
  long long ldg;
  const int64_t* order;    // [E] edge ids stably sorted by source
  const int64_t* seg_lo;   // [U] (null: no edges)
  const int64_t* seg_hi;   // [U]
  const int32_t* etgt;     // [E] target of every edge
  const float* sc;         // [E, H, 2]
  float* dk;               // [U, H*C], rows ldd apart
  float* dv;
  long long ldd;
  long long U, E;
  int H, C, G;
};

// the n_here (<= 64) edges whose ids and targets lanes 0 .. n_here - 1 hold, a block at a time, the next block requested ahead
template <int V, int VW>
__device__ __forceinline__ void tv_source_block(const TvSrcArgs& a, const TvLane& L, const int my_e, const int my_i, const int n_here, TvVec<V>& dk,
                                                TvVec<V>& dv) {
  constexpr int B = tv_block<V>();
  const float* __restrict__ qp = a.q + L.col;
  const float* __restrict__ gp = a.dout + L.col;
  const float* __restrict__ sp = a.sc + 2 * L.h;
  TvVec<V> qq[B], gg[B], qn[B], gn[B];
  float2 ss[B], sn[B];
  auto request = [&](int c0, TvVec<V> (&Q)[B], TvVec<V> (&Gg)[B], float2 (&S)[B]) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < B; ++s) {
      const int sl = c0 + s < n_here ? c0 + s : n_here - 1;
      const long long e = __builtin_amdgcn_readlane(my_e, sl), i = __builtin_amdgcn_readlane(my_i, sl);
      Q[s] = tv_load<V, VW>(qp + i * a.ldq, L.nv);
      Gg[s] = tv_load<V, VW>(gp + i * a.ldg, L.nv);
      S[s] = *reinterpret_cast<const float2*>(sp + e * 2 * a.H);
    }
  };
  request(0, qq, gg, ss);
  for (int c0 = 0; c0 < n_here; c0 += B) {
    const bool more = c0 + B < n_here;
    if (more) request(c0 + B, qn, gn, sn);
#pragma unroll
    for (int s = 0; s < B; ++s) {
      if (c0 + s < n_here) {  // wave-uniform
#pragma unroll
        for (int u = 0; u < V; ++u) {
          dk.f[u] = __fmaf_rn(ss[s].x, qq[s].f[u], dk.f[u]);
          dv.f[u] = __fmaf_rn(ss[s].y, gg[s].f[u], dv.f[u]);
        }
      }
    }
    if (more) {
#pragma unroll
      for (int s = 0; s < B; ++s) {
        qq[s] = qn[s];
        gg[s] = gn[s];
        ss[s] = sn[s];
      }
    }
  }
}

template <int V, int VW>
__global__ __launch_bounds__(256) void tconv_source_backward_kernel(const TvSrcArgs a) {
  __shared__ float s_dk[kTvWaves][kWave][V];
  __shared__ float s_dv[kTvWaves][kWave][V];
  const long long j = blockIdx.x;
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const long long lo = a.seg_lo ? a.seg_lo[j] : 0, hi = a.seg_lo ? a.seg_hi[j] : 0;
  const long long n = hi > lo ? hi - lo : 0;
  const bool split = n > kTvShort;  // (uniform over the workgroup)
  if (!split && wave) return;
  const TvLane L = tv_lane<V>(lane, a.H, a.C, a.G);
  TvVec<V> dk = tv_zero<V>(), dv = tv_zero<V>();
  if (!split) {
    if (n) {
      int my_e = 0, my_i = 0;
      if (lane < n) {
        my_e = tv_clamp(a.order[lo + lane], a.E);
        my_i = tv_clamp(a.etgt[my_e], a.U);
      }
      tv_source_block<V, VW>(a, L, my_e, my_i, (int)n, dk, dv);
    }
  } else {
    for (long long p0 = lo + wave; p0 < hi; p0 += (long long)kTvWaves * kWave) {
      const long long my_p = p0 + (long long)kTvWaves * lane;
      int my_e = 0, my_i = 0;
      if (my_p < hi) {
        my_e = tv_clamp(a.order[my_p], a.E);
        my_i = tv_clamp(a.etgt[my_e], a.U);
      }
      const long long left = (hi - p0 + kTvWaves - 1) / kTvWaves;
      tv_source_block<V, VW>(a, L, my_e, my_i, left < kWave ? (int)left : kWave, dk, dv);
    }
#pragma unroll
    for (int u = 0; u < V; ++u) {
      s_dk[wave][lane][u] = dk.f[u];
      s_dv[wave][lane][u] = dv.f[u];
    }
    __syncthreads();
    if (wave) return;
    dk = tv_zero<V>();
    dv = tv_zero<V>();
#pragma unroll
    for (int w2 = 0; w2 < kTvWaves; ++w2) {
#pragma unroll
      for (int u = 0; u < V; ++u) {
        dk.f[u] += s_dk[w2][lane][u];
        dv.f[u] += s_dv[w2][lane][u];
      }
    }
  }
  tv_store<V, VW>(a.dk + j * a.ldd + L.col, L.nv, dk);
  tv_store<V, VW>(a.dv + j * a.ldd + L.col, L.nv, dv);
}

__global__ __launch_bounds__(256) void tv_fill_zero_kernel(float* __restrict__ p, long long n) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += step) p[x] = 0.f;
}

// the widest access every row piece allows: C and the leading dimensions multiples of it, the pointers aligned to it
static int tv_width(int V, int C, uintptr_t ptr_bits, long long ld_bits) {
  if (V >= 4 && C % 4 == 0 && (ptr_bits & 15) == 0 && (ld_bits & 3) == 0) return 4;
  if (V <= 4 && C % 2 == 0 && (ptr_bits & 7) == 0 && (ld_bits & 1) == 0) return 2;
  return 1;
}

#define TV_DISPATCH(KERNEL, V, VW, grid, st, args)                                                          \
  do {                                                                                                      \
    const dim3 block__(256);                                                                                \
    if (V == 2 && VW == 2) hipLaunchKernelGGL((KERNEL<2, 2>), grid, block__, 0, st, args);                  \
    else if (V == 2) hipLaunchKernelGGL((KERNEL<2, 1>), grid, block__, 0, st, args);                        \
    else if (V == 4 && VW == 4) hipLaunchKernelGGL((KERNEL<4, 4>), grid, block__, 0, st, args);             \
    else if (V == 4 && VW == 2) hipLaunchKernelGGL((KERNEL<4, 2>), grid, block__, 0, st, args);             \
    else if (V == 4) hipLaunchKernelGGL((KERNEL<4, 1>), grid, block__, 0, st, args);                        \
    else if (V == 8 && VW == 4) hipLaunchKernelGGL((KERNEL<8, 4>), grid, block__, 0, st, args);             \
    else if (V == 8) hipLaunchKernelGGL((KERNEL<8, 1>), grid, block__, 0, st, args);                        \
    else if (VW == 4) hipLaunchKernelGGL((KERNEL<16, 4>), grid, block__, 0, st, args);                      \
    else hipLaunchKernelGGL((KERNEL<16, 1>), grid, block__, 0, st, args);                                   \
  } while (0)

static int tv_unsupported(const char* what, int H, int C) {
  set_error("%s: heads = %d, out_channels = %d is outside the training envelope (C <= %d, H <= %d, H C <= %d)", what, H, C, kTvMaxC, kTvMaxH, kTvMaxHC);
  return TGMX_E_UNSUPPORTED;
}

// The attention backward with explicit leading dimensions (the layer writes dq | dk | dv side by side and has dout copied behind them).
// dry: lay the workspace out only.
struct TvAttendCall {
  const float *q, *k, *v;
  long long ldq;
  const float* eproj;
  const int64_t *order, *src, *seg_lo, *seg_hi;
  long long U, E;
  int H, C;
  float scale;
  const float* dout;
  long long ldg;
  float *dq, *dk, *dv, *gcopy;
  long long ldd;
  float* de;
  DropoutArgs drop;
};

static int tv_attend_pass(const TvAttendCall& c, void* workspace, bool dry, size_t* need, tgmx_stream_t stream) {
  const long long U = c.U, E = c.E;
  const size_t e1 = E > 0 ? (size_t)E : 1;
  WorkspaceCarver ws(dry ? nullptr : workspace);
  float* sc = ws.take<float>(e1 * 2 * c.H);
  int32_t* etgt = ws.take<int32_t>(e1);
  int64_t* order_s = ws.take<int64_t>(e1);
  int64_t* sseg_lo = ws.take<int64_t>((size_t)U);
  int64_t* sseg_hi = ws.take<int64_t>((size_t)U);
  int32_t* status = ws.take<int32_t>(1);
  const size_t sort_bytes = E > 0 ? tgmx_segment_sort_workspace_bytes(E) : 0;
  char* sort_ws = ws.take<char>(sort_bytes);
  *need = ws.total();
  if (dry) return TGMX_OK;

  const TvLayout lay = tv_layout(c.H, c.C);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)U);
  const bool edges = E > 0;
  int rc;
  {
    TvArgs a{};
    a.q = c.q; a.k = c.k; a.v = c.v; a.ldq = c.ldq; a.eproj = c.eproj; a.order = c.order; a.src = c.src;
    a.seg_lo = edges ? c.seg_lo : nullptr; a.seg_hi = c.seg_hi; a.dout = c.dout; a.ldg = c.ldg; a.dq = c.dq; a.gcopy = c.gcopy; a.ldd = c.ldd;
    a.de = c.de; a.sc = sc; a.etgt = etgt; a.status_zero = status; a.U = U; a.E = E; a.H = c.H; a.C = c.C; a.G = lay.G; a.scale = c.scale; a.drop = c.drop;
    const uintptr_t bits = (uintptr_t)c.q | (uintptr_t)c.k | (uintptr_t)c.v | (uintptr_t)c.eproj | (uintptr_t)c.dout | (uintptr_t)c.dq |
                           (uintptr_t)c.gcopy | (uintptr_t)c.de;
    const int VW = tv_width(lay.V, c.C, bits, c.ldq | c.ldg | c.ldd);
    TV_DISPATCH(tconv_target_backward_kernel, lay.V, VW, grid, st, a);
    TGMX_CHECK_LAUNCH("tconv_target_backward");
  }
  if (edges && (rc = tgmx_segment_sort(c.src, E, (int32_t)U, order_s, sseg_lo, sseg_hi, sort_ws, sort_bytes, status, stream))) return rc;
  {
    const TvSrcArgs a{c.q, c.ldq, c.dout, c.ldg, order_s, edges ? sseg_lo : nullptr, sseg_hi, etgt, sc, c.dk, c.dv, c.ldd, U, E, c.H, c.C, lay.G};
    const uintptr_t bits = (uintptr_t)c.q | (uintptr_t)c.dout | (uintptr_t)c.dk | (uintptr_t)c.dv;
    const int VW = tv_width(lay.V, c.C, bits, c.ldq | c.ldg | c.ldd);
    TV_DISPATCH(tconv_source_backward_kernel, lay.V, VW, grid, st, a);
    TGMX_CHECK_LAUNCH("tconv_source_backward");
  }
  return TGMX_OK;
}

static int tv_clear(float* p, size_t n, hipStream_t st) {
  if (!p || !n) return TGMX_OK;
  long long blocks = ((long long)n + 255) / 256;
  hipLaunchKernelGGL(tv_fill_zero_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, st, p, (long long)n);
  TGMX_CHECK_LAUNCH("tconv_backward(zero)");
  return TGMX_OK;
}

}  // namespace tgmx

using namespace tgmx;

extern "C" int tgmx_tconv_train_supported(int32_t H, int32_t C) { return tv_supported(H, C) ? 1 : 0; }

extern "C" size_t tgmx_tconv_attend_backward_det_workspace_bytes(int64_t U, int64_t E, int32_t H) {
  if (U < 0 || E < 0 || H < 1 || H > kTvMaxH) return 0;
  TvAttendCall c{};
  c.U = U; c.E = E; c.H = H; c.C = 1;
  size_t need = 0;
  tv_attend_pass(c, nullptr, true, &need, nullptr);
  return need;
}

extern "C" int tgmx_tconv_attend_backward_det(const float* q, const float* k, const float* v, const float* eproj, const int64_t* order,
                                              const int64_t* src, const int64_t* seg_lo, const int64_t* seg_hi, int64_t U, int64_t E, int32_t H,
                                              int32_t C, float scale, const float* dout, float* dq, float* dk, float* dv, float* de,
                                              const tgmx_dropout_t* drop, void* workspace, size_t workspace_bytes, tgmx_stream_t stream) {
  if (!tv_supported(H, C)) return tv_unsupported("tconv_attend_backward_det", H, C);
  TGMX_REQUIRE(U >= 0 && U < (1ll << 31) && E >= 0 && E < (1ll << 31), "tconv_attend_backward_det: bad sizes");
  if (U == 0) return TGMX_OK;
  TGMX_REQUIRE(q && dout && dq && dk && dv, "tconv_attend_backward_det: null pointer");
  TGMX_REQUIRE(E == 0 || (k && v && eproj && order && src && seg_lo && seg_hi && de), "tconv_attend_backward_det: null pointer (edges)");
  const long long HC = (long long)H * C;
  TvAttendCall c{q, k, v, HC, eproj, order, src, seg_lo, seg_hi, U, E, H, C, scale, dout, HC, dq, dk, dv, nullptr, HC, de, make_dropout(drop)};
  size_t need = 0;
  tv_attend_pass(c, nullptr, true, &need, nullptr);
  TGMX_REQUIRE(workspace && workspace_bytes >= need, "tconv_attend_backward_det: workspace too small (%zu bytes, %zu needed)", workspace_bytes, need);
  return tv_attend_pass(c, workspace, false, &need, stream);
}

// ---- the whole layer as one call --------------------------------------------------------------------------------------------------------------
static int tconv_backward_pass(const tgmx_tconv_bwd_t* a, bool dry, size_t* need, tgmx_stream_t stream) {
  const int64_t U = a->U, E = a->E;
  const int H = a->H, C = a->C, HC = H * C, T = a->T, Wd = a->T + a->D, in = a->in_ch;
  const bool edges = E > 0;
  const bool want_time = edges && a->d_time;
  const bool want_e = edges && (a->d_Wedge || a->d_time);
  hipStream_t st = (hipStream_t)stream;
  WorkspaceCarver ws(dry ? nullptr : a->workspace);
  const size_t e1 = edges ? (size_t)E : 1;
  float* d4 = ws.take<float>((size_t)U * 4 * HC);
  float* de = ws.take<float>(e1 * HC);
  int64_t* order = ws.take<int64_t>(e1);
  int64_t* seg_lo = ws.take<int64_t>((size_t)U);
  int64_t* seg_hi = ws.take<int64_t>((size_t)U);
  int32_t* status = ws.take<int32_t>(1);
  const size_t sort_bytes = edges ? tgmx_segment_sort_workspace_bytes(E) : 0;
  char* sort_ws = ws.take<char>(sort_bytes);
  TvAttendCall c{};
  c.U = U; c.E = E; c.H = H; c.C = C;
  size_t attend_bytes = 0;
  tv_attend_pass(c, nullptr, true, &attend_bytes, nullptr);
  char* attend_ws = ws.take<char>(attend_bytes);
  float* d_attr = ws.take<float>(want_time ? (size_t)E * T : 0);
  float* part = ws.take<float>(want_time ? (size_t)E * 2 * T : 0);
  size_t tn_bytes = tgmx_sgemm_tn_workspace_bytes(U, HC, in, 4);
  const size_t tn_e = edges ? tgmx_sgemm_tn_workspace_bytes(E, HC, Wd, 1) : 0;
  tn_bytes = tn_bytes > tn_e ? tn_bytes : tn_e;
  float* tn_ws = ws.take<float>(tn_bytes / sizeof(float) + 1);
  const int widest = 4 * HC > 2 * T ? 4 * HC : 2 * T;
  float* cs_ws = ws.take<float>((size_t)256 * widest);
  *need = ws.total();
  if (dry) return TGMX_OK;

  int rc;
  // 1. the attention backward over segments in ascending edge id (the forward's counting grouping leaves a segment in the order its
  //    atomics fell: the grouping is redone here by the stable sort, whose status word the small zero launch clears)
  if (edges) {
    if ((rc = tv_clear(reinterpret_cast<float*>(status), 1, st))) return rc;
    if ((rc = tgmx_segment_sort(a->tgt, E, (int32_t)U, order, seg_lo, seg_hi, sort_ws, sort_bytes, status, stream))) return rc;
  }
  const float* q = a->qkvs;
  c = TvAttendCall{q, q + U * HC, q + 2 * U * HC, HC, a->eproj, order, a->src, seg_lo, seg_hi, U, E, H, C, 1.0f / sqrtf((float)C), a->g, a->ldg,
                   d4, d4 + HC, d4 + 2 * HC, d4 + 3 * HC, 4ll * HC, de, make_dropout(&a->drop)};
  if ((rc = tv_attend_pass(c, attend_ws, false, &attend_bytes, stream))) return rc;
  // 2., 3. the edge projection and the time encoder behind it
  if (!want_e) {
    if ((rc = tv_clear(a->d_Wedge, (size_t)HC * Wd, st)) || (rc = tv_clear(a->d_time, (size_t)2 * T, st))) return rc;
  } else {
    if (a->d_Wedge && (rc = tgmx_sgemm_tn(de, HC, a->edge_attr, Wd, a->d_Wedge, Wd, E, HC, Wd, 1, 0, 0, 0, 0, tn_ws, stream))) return rc;
    if (a->d_time) {
      if ((rc = tgmx_sgemm_nt(de, HC, a->WeT, HC, d_attr, T, E, T, HC, nullptr, 0, 1, 0, 0, 0, stream))) return rc;
      if ((rc = tgmx_tconv_edge_attr_backward(a->last_update_local, a->src, a->t, a->tw, a->tb, d_attr, T, 0, E, part, stream))) return rc;
      if ((rc = tgmx_colsum(part, 2 * T, E, 2 * T, a->d_time, 0, cs_ws, stream))) return rc;
    }
  }
  // 4. the four node projections: d4 = dq | dk | dv | g against the same x
  if (a->d_W4 && (rc = tgmx_sgemm_tn(d4, 4 * HC, a->x, in, a->d_W4, in, U, HC, in, 4, HC, 0, (long long)HC * in, 0, tn_ws, stream))) return rc;
  if (a->d_b4 && (rc = tgmx_colsum(d4, 4 * HC, U, 4 * HC, a->d_b4, 0, cs_ws, stream))) return rc;
  if (a->d_x && (rc = tgmx_sgemm_nt(d4, 4 * HC, a->W4T, 4 * HC, a->d_x, in, U, in, 4 * HC, nullptr, 0, 1, 0, 0, 0, stream))) return rc;
  return TGMX_OK;
}

static int tconv_bwd_check(const tgmx_tconv_bwd_t* a, const char* what) {
  TGMX_REQUIRE(a, "%s: null argument block", what);
  if (!tv_supported(a->H, a->C)) return tv_unsupported(what, a->H, a->C);
  TGMX_REQUIRE(a->U >= 0 && a->U < (1ll << 31) && a->E >= 0 && a->E < (1ll << 31) && a->in_ch > 0 && a->T > 0 && a->D >= 0, "%s: bad sizes", what);
  TGMX_REQUIRE(a->ldg >= a->H * a->C || a->U == 0, "%s: leading dimension of the upstream gradient", what);
  return TGMX_OK;
}

extern "C" size_t tgmx_tconv_backward_workspace_bytes(const tgmx_tconv_bwd_t* a) {
  size_t need = 0;
  if (tconv_bwd_check(a, "tconv_backward_workspace_bytes") != TGMX_OK) return 0;
  return tconv_backward_pass(a, true, &need, nullptr) == TGMX_OK ? need : 0;
}

extern "C" int tgmx_tconv_backward(const tgmx_tconv_bwd_t* a, tgmx_stream_t stream) {
  int rc;
  if ((rc = tconv_bwd_check(a, "tconv_backward"))) return rc;
  if (a->U == 0) return TGMX_OK;
  const bool edges = a->E > 0;
  TGMX_REQUIRE(a->g && a->qkvs, "tconv_backward: the upstream gradient or the forward's saved buffers are missing");
  TGMX_REQUIRE(!edges || (a->eproj && a->src && a->tgt), "tconv_backward: the forward's edge buffers are missing");
  TGMX_REQUIRE(!a->d_W4 || a->x, "tconv_backward: d_W4 needs x");
  TGMX_REQUIRE(!a->d_x || a->W4T, "tconv_backward: d_x needs the transposed stacked weights");
  TGMX_REQUIRE(!(edges && a->d_Wedge) || a->edge_attr, "tconv_backward: d_Wedge needs edge_attr");
  TGMX_REQUIRE(!(edges && a->d_time) || (a->WeT && a->last_update_local && a->t && a->tw && a->tb), "tconv_backward: d_time needs the time encoder's inputs");
  size_t need = 0;
  if ((rc = tconv_backward_pass(a, true, &need, nullptr))) return rc;
  TGMX_REQUIRE(a->workspace && a->workspace_bytes >= need, "tconv_backward: workspace too small (%zu bytes, %zu needed)", a->workspace_bytes, need);
  return tconv_backward_pass(a, false, &need, stream);
}
