// CTAN (tgm/nn/encoder/ctan.py): the memory's update_state and the encoder's inference forward.
//
//   tgmx_ctan_memory_update   CTANMemory.update_state (ctan.py:128-147) without `unique`, the dense [U, 2B] score matrix or any read
//                             back: two launches over the 2B positions of cat[src, pos_dst] and a per-node scratch table.
//   tgmx_ctan_attend          the attention of PyG's TransformerConv(heads=1, root_weight=False) for a WIDE head (C <= 256): one wave covers
//                             the whole row, with AntiSymmetricConv's update x <- x + eps tanh(phi + x A^T + b) as its epilogue.
//   tgmx_ctan_forward         CTAN.forward as one call: what does not change over AntiSymmetricConv's iterations (edge encoding, edge
//                             projection, grouping by target) runs once, an iteration is one batched GEMM and one attention launch.
#include <math.h>

#include "common.h"
#include "ctan_rows.h"
#include "lanes.h"

namespace tgmx {

// ---------------------------------------------------------------------------------------------------------------------------------
// Memory.  LastAggregator (tgn.py:43-56) takes, per node, the FIRST position among those with the largest float32(t); last_update is
// the exact int64 maximum.  Launch 1 folds every position into its node's scratch entry with two atomic maxima: the packed key
// {float32(t) as an ordered 32-bit pattern | ~p} (the larger time wins, then the smaller position) and the int64 time.  Launch 2: one
// wave per position; the position its node's key names copies its embedding row, writes last_update and puts the entry back to its
// rest value -- every other position of that node reads either the key (not its own) or the rest value (nobody's) and does nothing,
// so the table is clean again when the call ends.  Maxima commute: the same bits whatever the order the atomics land in.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr long long kCtanTimeRest = (long long)0x8000000000000000ull;  // INT64_MIN, the rest value of tmax; the key's is 0

struct CtanMemArgs {
  const void* src;
  const void* dst;
  int src64, dst64;
  const int64_t* t;
  long long B;
  const float* src_emb;
  const float* dst_emb;
  long long rows_src;  // rows of src_emb: row p of cat[src_emb, pos_dst_emb] is pos_dst_emb's row p - rows_src beyond them
  int M;
  long long N;
  float* memory;
  int64_t* last_update;
  unsigned long long* key;
  long long* tmax;
  int32_t* status;
};

__device__ __forceinline__ long long ctan_node(const CtanMemArgs& a, long long p) {
  const bool first = p < a.B;
  const void* ids = first ? a.src : a.dst;
  const long long r = first ? p : p - a.B;
  return (first ? a.src64 : a.dst64) ? (long long)reinterpret_cast<const int64_t*>(ids)[r] : (long long)reinterpret_cast<const int32_t*>(ids)[r];
}

__device__ __forceinline__ unsigned long long ctan_key(long long t, long long p) {
  const unsigned f = __float_as_uint((float)t);                  // round to nearest even, as Tensor.float() does
  const unsigned ordered = (f & 0x80000000u) ? ~f : (f | 0x80000000u);  // unsigned order == float order
  return ((unsigned long long)ordered << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)p);
}

__global__ __launch_bounds__(256) void ctan_mem_scan_kernel(const CtanMemArgs a) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= 2 * a.B) return;
  const long long node = ctan_node(a, p);
  if (node < 0 || node >= a.N) {
    atomicOr(a.status, 1);
    return;
  }
  const long long t = a.t[p < a.B ? p : p - a.B];
  atomicMax(&a.key[node], ctan_key(t, p));
  atomicMax(&a.tmax[node], t);
}

__global__ __launch_bounds__(256) void ctan_mem_commit_kernel(const CtanMemArgs a) {
  const long long p = (long long)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x >> 6);
  if (p >= 2 * a.B) return;
  const long long node = ctan_node(a, p);
  if (node < 0 || node >= a.N) return;
  const unsigned long long key = __atomic_load_n(&a.key[node], __ATOMIC_RELAXED);
  if ((unsigned)(key & 0xFFFFFFFFull) != 0xFFFFFFFFu - (unsigned)p) return;  // another position of this node won (or has won and tidied up)
  const float* __restrict__ row = p < a.rows_src ? a.src_emb + p * a.M : a.dst_emb + (p - a.rows_src) * a.M;
  float* __restrict__ mem = a.memory + node * a.M;
  for (int c = lane_id(); c < a.M; c += kWave) mem[c] = row[c];
  if (lane_id() == 0) {
    a.last_update[node] = a.tmax[node];
    a.tmax[node] = kCtanTimeRest;
    __atomic_store_n(&a.key[node], 0ull, __ATOMIC_RELAXED);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Edge encoding (ctan.py:73-76): edge_attr[e] = [msg[e] | cos(rel w + b)], rel = (float(|last_update[src] - t|) - mean) / std in float32
// -- the message FIRST (TGN's layer has the time part first).  The thread of an edge's first column also writes the edge's source,
// clamped into [0, U) (flagged in *status like an out-of-range target), for the attention to read.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctan_edge_attr_kernel(const int64_t* __restrict__ lu, const int64_t* __restrict__ src,
                                                             const int64_t* __restrict__ t, const float* __restrict__ msg,
                                                             const float* __restrict__ tw, const float* __restrict__ tb, int T, int D, long long E,
                                                             long long U, float mean, float std, float* __restrict__ out,
                                                             int64_t* __restrict__ src_ok, int32_t* status) {
  const int W = D + T;
  const long long total = E * W;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += step) {
    const long long e = x / W;
    const int c = (int)(x - e * W);
    long long j = src[e];
    if (j < 0 || j >= U) {
      if (c == 0) atomicOr(status, TGMX_ST_EDGE_RANGE);
      j = j < 0 ? 0 : U - 1;
    }
    if (c == 0) src_ok[e] = j;
    float v;
    if (c < D) {
      v = msg[e * D + c];
    } else {
      long long d = lu[j] - t[e];
      if (d < 0) d = -d;
      const float rel = ((float)d - mean) / std;
      v = cos_t2v(__fmaf_rn(rel, tw[c - D], tb[c - D]));
    }
    out[x] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Attention for H = 1 and a wide head.  Lane l owns the V = ceil(C / 64) <= 4 consecutive columns [V l, V l + V) of every row it touches
// (VEC: one 16- / 8-byte load, C a multiple of V and the rows so aligned; otherwise V scalar loads with a tail: C = 5, 100 over 3, ...).
// The walk is tconv_walk_block's (csrc/tgn.hip): a segment's edges go through in blocks of four whose 12 row pieces -- k and v of the source,
// the edge projection -- are ALL requested before the previous block is scored; here a score is a butterfly over all 64 lanes (DPP and the
// gfx950 half-wave swaps, no LDS), so every lane holds the softmax state and weights its own columns.  A segment of up to kCtanShort edges
// is wave 0's alone; a longer one is split over the workgroup's four waves (wave w takes positions w, w + 4, ...) whose states meet in LDS
// and are merged in wave order.  The sums run in ascending edge id on every path: two runs give the same bits.
// Every target goes through the epilogue on wave 0, one without incoming edges with phi = 0:
//   mode 0   h4 += phi                              (what tgmx_tconv_attend leaves: for tests and A/B timing against it)
//   mode 1   x <- x + eps tanh(h4 + phi)            (AntiSymmetricConv, h4 = x A^T + bias from the batched projection)
//   mode 2   out = tanh(x + eps tanh(h4 + phi))     (the last iteration, with CTAN's final tanh)
// (CtanAttendArgs, the row pieces and the walk: ctan_rows.h, shared with the backward.  x_next: mode 1 leaves x alone and writes the new
// x there -- the saving forward keeps every iteration's x.)
// ---------------------------------------------------------------------------------------------------------------------------------
template <int V, bool VEC>
__global__ __launch_bounds__(256) void ctan_attend_kernel(const CtanAttendArgs a) {
  __shared__ float s_m[kCtanWaves], s_l[kCtanWaves];
  __shared__ float s_acc[kCtanWaves][kWave][V];
  const long long i = blockIdx.x;
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const long long lo = a.seg_lo[i], hi = a.seg_hi[i];
  const long long n = hi > lo ? hi - lo : 0;
  const bool split = n > kCtanShort;  // (uniform over the workgroup: the barrier below is reached by all four waves or by none)
  if (!split && wave) return;
  const long long C = a.C;
  int nv = a.C - lane * V;
  nv = nv < 0 ? 0 : (nv > V ? V : nv);
  const int col = nv ? lane * V : 0;
  const CtVec<V> q = ct_load<V, VEC>(a.q + i * C + col, nv);
  CtanWalk<V> st;
  st.m = -__builtin_inff();
  st.l = 0.f;
#pragma unroll
  for (int u = 0; u < V; ++u) st.acc.f[u] = 0.f;
  if (!split) {
    if (n) {
      int my_e = 0, my_j = 0;
      if (lane < n) {
        my_e = (int)a.order[lo + lane];  // (edge ids and local node ids of one batch: far below 2^31)
        my_j = (int)a.src[my_e];
      }
      ctan_walk_block<V, VEC>(a, q, nv, col, my_e, my_j, (int)n, st);
    }
  } else {
    for (long long p0 = lo + wave; p0 < hi; p0 += (long long)kCtanWaves * kWave) {
      const long long my_p = p0 + (long long)kCtanWaves * lane;
      int my_e = 0, my_j = 0;
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
    if (wave) return;
    float M = s_m[0];
#pragma unroll
    for (int w2 = 1; w2 < kCtanWaves; ++w2) M = fmaxf(M, s_m[w2]);
    float L = 0.f;
    CtVec<V> A;
#pragma unroll
    for (int u = 0; u < V; ++u) A.f[u] = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < kCtanWaves; ++w2) {
      const float f = s_l[w2] > 0.f ? expf(s_m[w2] - M) : 0.f;  // a wave without edges has m = -inf, l = 0
      L += s_l[w2] * f;
#pragma unroll
      for (int u = 0; u < V; ++u) A.f[u] += s_acc[w2][lane][u] * f;
    }
    st.l = L;
    st.acc = A;
  }
  // wave 0: the row's epilogue
  CtVec<V> r = ct_load<V, VEC>(a.h4 + i * C + col, nv);
  if (n) {
#pragma unroll
    for (int u = 0; u < V; ++u) r.f[u] += st.acc.f[u] / st.l;
  }
  if (a.mode == 0) {
    if (n) ct_store<V, VEC>(a.h4 + i * C + col, nv, r);
    return;
  }
  CtVec<V> xv = ct_load<V, VEC>(a.x + i * C + col, nv);
#pragma unroll
  for (int u = 0; u < V; ++u) {
    xv.f[u] = __fmaf_rn(a.eps, tanhf(r.f[u]), xv.f[u]);
    if (a.mode == 2) xv.f[u] = tanhf(xv.f[u]);
  }
  ct_store<V, VEC>((a.mode == 2 ? a.out : (a.x_next ? a.x_next : a.x)) + i * C + col, nv, xv);
}

// the epilogue alone (h4 already holds x A^T + bias + phi): a head wider than kCtanMaxC, whose attention is tgmx_tconv_attend's, or no edges
__global__ __launch_bounds__(256) void ctan_epilogue_kernel(const float* h4, const float* x, float* x_next, float* __restrict__ out,
                                                            long long total, float eps, int mode) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += step) {
    float xv = __fmaf_rn(eps, tanhf(h4[p]), x[p]);
    if (mode == 2) out[p] = tanhf(xv);
    else x_next[p] = xv;
  }
}

static int ctan_epilogue(const float* h4, float* x, float* x_next, float* out, long long total, float eps, int mode, hipStream_t st) {
  long long blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(ctan_epilogue_kernel, dim3((unsigned)blocks), dim3(256), 0, st, h4, x, x_next ? x_next : x, out, total, eps, mode);
  TGMX_CHECK_LAUNCH("ctan_epilogue");
  return TGMX_OK;
}

static int ctan_attend_launch(const CtanAttendArgs& a, hipStream_t st) {
  const int V = (a.C + kWave - 1) / kWave;
  uintptr_t bits = (uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.eproj | (uintptr_t)a.h4;
  if (a.mode) bits |= (uintptr_t)a.x;
  if (a.mode == 2) bits |= (uintptr_t)a.out;
  if (a.mode == 1 && a.x_next) bits |= (uintptr_t)a.x_next;
  const dim3 grid((unsigned)a.U), block(256);
  if (V == 4 && a.C % 4 == 0 && (bits & 15) == 0) hipLaunchKernelGGL((ctan_attend_kernel<4, true>), grid, block, 0, st, a);
  else if (V == 4) hipLaunchKernelGGL((ctan_attend_kernel<4, false>), grid, block, 0, st, a);
  else if (V == 3) hipLaunchKernelGGL((ctan_attend_kernel<3, false>), grid, block, 0, st, a);
  else if (V == 2 && a.C % 2 == 0 && (bits & 7) == 0) hipLaunchKernelGGL((ctan_attend_kernel<2, true>), grid, block, 0, st, a);
  else if (V == 2) hipLaunchKernelGGL((ctan_attend_kernel<2, false>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((ctan_attend_kernel<1, false>), grid, block, 0, st, a);
  TGMX_CHECK_LAUNCH("ctan_attend");
  return TGMX_OK;
}

}  // namespace tgmx

using namespace tgmx;

extern "C" int tgmx_ctan_memory_update(const void* src, int32_t src_is64, const void* dst, int32_t dst_is64, const int64_t* t, int64_t B,
                                       const float* src_emb, const float* dst_emb, int64_t rows_src, int32_t M, int64_t num_nodes, float* memory,
                                       int64_t* last_update, void* scratch_key, int64_t* scratch_tmax, int32_t* status, tgmx_stream_t stream) {
  TGMX_REQUIRE(B >= 0 && M > 0 && num_nodes > 0 && rows_src >= 0, "ctan_memory_update: bad sizes");
  TGMX_REQUIRE(2 * B < (1ll << 31), "ctan_memory_update: more than 2^31 positions");
  if (B == 0) return TGMX_OK;
  TGMX_REQUIRE(src && dst && t && (src_emb || rows_src == 0) && dst_emb && memory && last_update && scratch_key && scratch_tmax && status,
               "ctan_memory_update: null pointer");
  const CtanMemArgs a{src, dst, src_is64 ? 1 : 0, dst_is64 ? 1 : 0, t, B, src_emb, dst_emb, rows_src, M, num_nodes, memory, last_update,
                      reinterpret_cast<unsigned long long*>(scratch_key), reinterpret_cast<long long*>(scratch_tmax), status};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ctan_mem_scan_kernel, dim3((unsigned)((2 * B + 255) / 256)), dim3(256), 0, st, a);
  TGMX_CHECK_LAUNCH("ctan_memory_update(scan)");
  hipLaunchKernelGGL(ctan_mem_commit_kernel, dim3((unsigned)((2 * B + 3) / 4)), dim3(256), 0, st, a);
  TGMX_CHECK_LAUNCH("ctan_memory_update(commit)");
  return TGMX_OK;
}

static int ctan_attend(const float* q, const float* k, const float* v, const float* eproj, const int64_t* order, const int64_t* src,
                       const int64_t* seg_lo, const int64_t* seg_hi, int64_t U, int32_t C, float scale, float* h4, float* x, float* x_next, float* out,
                       float epsilon, int32_t mode, tgmx_stream_t stream) {
  TGMX_REQUIRE(U >= 0 && C > 0 && mode >= 0 && mode <= 2, "ctan_attend: bad sizes");
  if (U == 0) return TGMX_OK;
  TGMX_REQUIRE(q && k && v && eproj && order && src && seg_lo && seg_hi && h4 && (mode == 0 || x) && (mode != 2 || out), "ctan_attend: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (C > kCtanMaxC) {  // wider than a wave covers with four columns a lane: the generic walk, then the epilogue on its own
    const int rc = tgmx_tconv_attend(q, k, v, eproj, order, src, seg_lo, seg_hi, U, 1, C, scale, h4, nullptr, stream);
    if (rc || mode == 0) return rc;
    return ctan_epilogue(h4, x, x_next, out, (long long)U * C, epsilon, mode, st);
  }
  return ctan_attend_launch(CtanAttendArgs{q, k, v, eproj, order, src, seg_lo, seg_hi, h4, x, out, U, C, scale, epsilon, mode, x_next}, st);
}

extern "C" int tgmx_ctan_attend(const float* q, const float* k, const float* v, const float* eproj, const int64_t* order, const int64_t* src,
                                const int64_t* seg_lo, const int64_t* seg_hi, int64_t U, int32_t C, float scale, float* h4, float* x, float* out,
                                float epsilon, int32_t mode, tgmx_stream_t stream) {
  return ctan_attend(q, k, v, eproj, order, src, seg_lo, seg_hi, U, C, scale, h4, x, nullptr, out, epsilon, mode, stream);
}

extern "C" int tgmx_ctan_forward(const tgmx_ctan_fwd_t* a, tgmx_stream_t stream) {
  TGMX_REQUIRE(a, "ctan_forward: null argument block");
  const int64_t U = a->U, E = a->E;
  const int M = a->M, Wd = a->D + a->T;
  TGMX_REQUIRE(U >= 0 && E >= 0 && M > 0 && a->in_ch > 0 && a->T > 0 && a->D >= 0 && a->num_iters >= 0, "ctan_forward: bad sizes");
  if (U == 0) return TGMX_OK;
  TGMX_REQUIRE(a->node_x && a->W_x && a->b_x && a->W4 && a->b4 && (a->x || a->x_save) && a->qkvs && a->out, "ctan_forward: null pointer");
  // x_save: iteration `it` reads slot `it` and writes slot `it + 1` (the same kernels, the same bits); null: one x, updated in place
  const long long slot = a->x_save ? (long long)U * M : 0;
  float* x0 = a->x_save ? a->x_save : a->x;
  hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  // x = enc_x(node_x)
  if ((rc = tgmx_sgemm_nt(a->node_x, a->in_ch, a->W_x, a->in_ch, x0, M, U, M, a->in_ch, a->b_x, 0, 1, 0, 0, 0, stream))) return rc;
  if (E) {
    // once per call: nothing of this depends on x
    TGMX_REQUIRE(a->last_update && a->src && a->tgt && a->t && (a->D == 0 || a->msg) && a->tw && a->tb && a->W_edge && a->edge_attr && a->eproj &&
                     a->src_ok && a->order && a->seg_lo && a->seg_hi && a->sort_ws && a->status,
                 "ctan_forward: null pointer");
    long long blocks = (E * Wd + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(ctan_edge_attr_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a->last_update, a->src, a->t, a->msg, a->tw, a->tb, a->T, a->D,
                       (long long)E, (long long)U, a->mean_delta_t, a->std_delta_t, a->edge_attr, a->src_ok, a->status);
    TGMX_CHECK_LAUNCH("ctan_forward(edge_attr)");
    if ((rc = tgmx_sgemm_nt(a->edge_attr, Wd, a->W_edge, Wd, a->eproj, M, E, M, Wd, nullptr, 0, 1, 0, 0, 0, stream))) return rc;
    if ((rc = tgmx_segment_sort(a->tgt, E, (int32_t)U, a->order, a->seg_lo, a->seg_hi, a->sort_ws, a->sort_ws_bytes, a->status, stream))) return rc;
  }
  float* h4 = a->qkvs + 3 * U * M;
  const float scale = 1.0f / sqrtf((float)M);
  for (int it = 0; it < a->num_iters; ++it) {
    const int mode = it + 1 == a->num_iters ? 2 : 1;
    float* x = x0 + it * slot;
    float* x_next = a->x_save && mode == 1 ? x + slot : nullptr;
    // q | k | v | x A^T + bias: one batched problem over the stacked weights
    if ((rc = tgmx_sgemm_nt(x, M, a->W4, M, a->qkvs, M, U, M, M, a->b4, 0, 4, 0, (long long)M * M, U * M, stream))) return rc;
    if (E) rc = ctan_attend(a->qkvs, a->qkvs + U * M, a->qkvs + 2 * U * M, a->eproj, a->order, a->src_ok, a->seg_lo, a->seg_hi, U, M, scale, h4, x, x_next,
                            a->out, a->epsilon, mode, stream);
    else rc = ctan_epilogue(h4, x, x_next, a->out, (long long)U * M, a->epsilon, mode, st);
    if (rc) return rc;
  }
  if (a->num_iters == 0) return ctan_epilogue(x0, x0, nullptr, a->out, (long long)U * M, 0.f, 2, st);  // no iteration: tanh(enc_x(node_x))
  return TGMX_OK;
}
