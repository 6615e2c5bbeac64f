// The wide-head row pieces CTAN's attention (csrc/ctan.hip) and its backward (csrc/ctan_bwd.hip) share: the lane's piece of a row, the
// block-of-four walk over a target's incoming edges, and the argument block of the forward launch.
#pragma once
#include "common.h"
#include "lanes.h"

namespace tgmx {

struct CtanAttendArgs {
  const float *q, *k, *v;  // [U, C]
  const float* eproj;      // [E, C], original edge order
  const int64_t* order;    // [E] edge ids stably sorted by target
  const int64_t* src;      // [E] source of every edge, in [0, U)
  const int64_t* seg_lo;   // [U]
  const int64_t* seg_hi;   // [U]
  float* h4;               // [U, C]
  float* x;                // [U, C] (modes 1, 2)
  float* out;              // [U, C] (mode 2)
  long long U;
  int C;
  float scale, eps;
  int mode;
  float* x_next;           // [U, C] mode 1 writes the new x here; null: in place, over x
};

constexpr int kCtanShort = 16;
constexpr int kCtanWaves = 4;
constexpr int kCtanMaxC = 4 * kWave;

template <int V>
struct CtVec {
  float f[V];
};
// the lane's piece of a row: p points at its first column, nv of its V columns exist (VEC: nv is 0 or V)
template <int V, bool VEC>
__device__ __forceinline__ CtVec<V> ct_load(const float* __restrict__ p, const int nv) {
  CtVec<V> r;
  if constexpr (VEC && V == 4) {
    const float4 x = nv ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
    r.f[0] = x.x; r.f[1] = x.y; r.f[2] = x.z; r.f[3] = x.w;
  } else if constexpr (VEC && V == 2) {
    const float2 x = nv ? *reinterpret_cast<const float2*>(p) : make_float2(0.f, 0.f);
    r.f[0] = x.x; r.f[1] = x.y;
  } else {
#pragma unroll
    for (int u = 0; u < V; ++u) r.f[u] = u < nv ? p[u] : 0.f;
  }
  return r;
}
template <int V, bool VEC>
__device__ __forceinline__ void ct_store(float* __restrict__ p, const int nv, const CtVec<V>& r) {
  if constexpr (VEC && V == 4) {
    if (nv) *reinterpret_cast<float4*>(p) = make_float4(r.f[0], r.f[1], r.f[2], r.f[3]);
  } else if constexpr (VEC && V == 2) {
    if (nv) *reinterpret_cast<float2*>(p) = make_float2(r.f[0], r.f[1]);
  } else {
#pragma unroll
    for (int u = 0; u < V; ++u)
      if (u < nv) p[u] = r.f[u];
  }
}

template <int V>
struct CtanWalk {
  float m, l;
  CtVec<V> acc;
};

// the n_here (<= 64) edges whose ids / sources lanes 0 .. n_here - 1 hold, in lane order, four at a time
template <int V, bool VEC>
__device__ __forceinline__ void ctan_walk_block(const CtanAttendArgs& a, const CtVec<V> q, const int nv, const int col, const int my_e, const int my_j,
                                                const int n_here, CtanWalk<V>& st) {
  const long long C = a.C;
  const float* __restrict__ kp = a.k + col;
  const float* __restrict__ vp = a.v + col;
  const float* __restrict__ ep = a.eproj + col;
  CtVec<V> kk[4], vv[4], ee[4], kn[4], vn[4], en[4];
  auto request = [&](int c0, CtVec<V> (&K)[4], CtVec<V> (&Vv)[4], CtVec<V> (&E)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int sl = c0 + s < n_here ? c0 + s : n_here - 1;  // (clamped: a position past the block re-reads its last edge, not used below)
      const long long e = __builtin_amdgcn_readlane(my_e, sl), j = __builtin_amdgcn_readlane(my_j, sl);
      K[s] = ct_load<V, VEC>(kp + j * C, nv);
      Vv[s] = ct_load<V, VEC>(vp + j * C, nv);
      E[s] = ct_load<V, VEC>(ep + e * C, nv);
    }
  };
  request(0, kk, vv, ee);
  float m = st.m, l = st.l;
  CtVec<V> acc = st.acc;
  for (int c0 = 0; c0 < n_here; c0 += 4) {
    const bool more = c0 + 4 < n_here;
    if (more) request(c0 + 4, kn, vn, en);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (c0 + s < n_here) {  // wave-uniform
        float p = q.f[0] * (kk[s].f[0] + ee[s].f[0]);
#pragma unroll
        for (int u = 1; u < V; ++u) p = __fmaf_rn(q.f[u], kk[s].f[u] + ee[s].f[u], p);
        p = lanes::butterfly_sum<1>(p);  // all 64 lanes (lanes past the row carry zeros)
        const float sc = p * a.scale;
        const float mn = sc > m ? sc : m;
        const float corr = expf(m - mn), w = expf(sc - mn);
#pragma unroll
        for (int u = 0; u < V; ++u) acc.f[u] = acc.f[u] * corr + w * (vv[s].f[u] + ee[s].f[u]);
        l = l * corr + w;
        m = mn;
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
  st.m = m;
  st.l = l;
  st.acc = acc;
}

}  // namespace tgmx
