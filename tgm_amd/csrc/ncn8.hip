// NCNPredictor at k = 8 (the reference's tgm/nn/decoder/ncnpred.py:192-315), for gfx950: the two-hop common-neighbour blocks of every pair
// from the sorted-row adjacency of ncn.hip, with no A A or A A A matrix and no [B, N] float matrix.
//
// One workgroup per pair (i, j).  Five int32 count rows over the N local ids:
//   R_i[n] = A[i, n], R_j[n] = A[j, n]            written once per distinct neighbour
//   S_i[n] = (A A)[i, n], S_j[n] = (A A)[j, n]    for every distinct neighbour m of the target, multiplicity a: row m is walked, +a per entry
//   sp[n]  = sum over m of R_i[m] R_j[m] A[m, n]  the same walk over the common neighbours, weight R_i[m] R_j[m]
// Integer adds only (LDS or L2 atomics), so the order of arrival cannot change a bit.  (R_i and R_j are rows too -- two more than the
// counts strictly need -- because the coefficient pass below wants both for EVERY n: two binary searches of dependent global loads per
// (pair, n) cost more than 8 N bytes of LDS.)  K3[i, i] = sum over the entries p of row i of S_i[cols[p]], K3[j, j] likewise, u = -A[i, j].
//
// Then the ids are taken 256 at a time, a thread each: the five coefficients c11, c12, c21, c22 (column masks, clamp) and sp in int64,
// converted once, the decay weight (float64) applied where a count is non-zero; the ids with a non-zero coefficient are compacted in ascending
// order (ballot order within a wave, wave order within the chunk) and every thread walks the chunk's list for ITS channel: five accumulators,
// kept in float64 -- the two-hop blocks sum hundreds of integer-weighted terms that cancel, where a float32 running sum alone is 1e-5 off (the
// reference's is) -- and rounded to float32 once.  No float atomics, one fixed order: two runs give the same bits.  tgmx_ncn8_forward's two
// Linear layers run in float64 for the same reason (ncn8_mlp_kernel).
//
// Storage: the rows live in LDS while N <= kNcn8LdsMaxN and are cleared per pair; above that the same kernel, templated on the storage, keeps
// them in a 5 N int32 region of the caller's workspace per resident workgroup, zeroed once per call and cleared per pair by walking the same
// rows again (never a memset per pair).  The counts are int32 and wrap silently beyond it: they are exact while every two-hop count
// S[n] = sum over m of A[t, m] A[m, n] and every sp[n] = sum over m of A[i, m] A[j, m] A[m, n] -- a sum of TRIPLE products of edge
// multiplicities, so three multi-edges of 1 300 copies each already pass it -- stays below 2^31 (the reference's float32 counts stop being
// exact at 2^24).  The products of two counts are formed in int64.
#include "common.h"
#include "edge_csr.h"
#include "ncn_rows.h"

#include <atomic>

namespace tgmx {

constexpr int kNcn8Threads = 256;
constexpr int kNcn8Waves = kNcn8Threads / kWave;
constexpr int kNcn8Rows = 5;
// LDS: a CU has 160 KiB (163 840 bytes) and a workgroup may take all of it.  A workgroup takes 20 N bytes of rows (dynamic) beside 8 272
// bytes of static chunk list (s_id 1 KiB, s_cf 5 KiB, s_w 2 KiB, s_cnt, s_k3): 150 KiB + 8.1 KiB at the cap of 7680 ids.  Workgroups (of
// 4 waves) per CU: ONE for 3683 <= N <= 7680, 2 up to N = 3682, 3 up to 2317, 4 up to 1634, 5 at the N = 1000 of a small batch, 8 up to
// N = 610.  The example's batch (B = 200 pairs) has fewer workgroups than the 256 CUs, so one resident workgroup per CU is all it can use.
constexpr int kNcn8LdsMaxN = 7680;
constexpr int kNcn8MaxGroups = 256;  // resident workgroups of the workspace form: one region each

struct Cn8Args {
  const float* x;
  long long N;
  int C;
  const int32_t* indptr;
  const int32_t* cols;
  const void* tar;
  int tar_is64;
  long long tar_stride, B;
  const int64_t* last_update;  // NULL: no time decay
  const int64_t* edge_time;
  const int32_t* last;  // NULL: every row keeps its adjacency row
  float* xs;
  long long ldxs;
  int32_t* ws;  // the workspace form's regions
  long long region;  // int32 per region
};

// the count rows: LDS, or a region of global memory that only this workgroup touches -- its atomics run in L2, so the reads go there too
// (agent-scope loads pass the CU's L1, which may hold the row as an earlier pair left it)
template <bool kLds>
struct Rows;
template <>
struct Rows<true> {
  static __device__ __forceinline__ int ld(const int32_t* p) { return *p; }
  static __device__ __forceinline__ void st(int32_t* p, int v) { *p = v; }
  static __device__ __forceinline__ void add(int32_t* p, int v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  static __device__ __forceinline__ void sync() { __syncthreads(); }
};
template <>
struct Rows<false> {
  static __device__ __forceinline__ int ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ void st(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ void add(int32_t* p, int v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ void sync() {
    __threadfence();
    __syncthreads();
  }
};

// W[r, n] with decay_weight's float32 argument (ncn_rows.h) and the exponential taken in float64: the weighted blocks multiply it onto
// integer counts in the hundreds and sum terms that cancel, where the rounding of a float32 weight shows in cn_emb
__device__ __forceinline__ double decay_weight_f64(const int64_t* __restrict__ last_update, long long et, long long n) {
  const float gap = (float)(et - (long long)last_update[n]);
  return exp(-(double)(gap / 10000.f));
}

// One target's side of the scatter: every wave takes distinct neighbours m of the target (the first entry of a run of equal ids; a = the
// run's length), writes R[m] = a and walks row m, its lanes an entry each: S[n] += a, and sp[n] += a b where m is a neighbour of the other
// target too (b entries in ITS row; `other` empty: no sp).  kClear: store zeros at the same places instead.
template <bool kLds, bool kClear>
__device__ __forceinline__ void ncn8_walk(const int32_t* __restrict__ indptr, const int32_t* __restrict__ cols, int lo, int hi, int olo, int ohi,
                                          int32_t* R, int32_t* S, int32_t* sp) {
  using Rw = Rows<kLds>;
  const int lane = lane_id(), wave = threadIdx.x / kWave;
  for (int p = lo + wave; p < hi; p += kNcn8Waves) {  // (p is the wave's: no divergence)
    const int m = cols[p];
    if (p > lo && cols[p - 1] == m) continue;
    const int a = lower_bound_i32(cols, p, hi, (long long)m + 1) - p;
    const int b = olo < ohi ? count_in(cols, olo, ohi, m) : 0;
    if (lane == 0) Rw::st(R + m, kClear ? 0 : a);
    const int mlo = indptr[m], mhi = indptr[m + 1];
    for (int q = mlo + lane; q < mhi; q += kWave) {
      const int n = cols[q];
      if (kClear) {
        Rw::st(S + n, 0);
        if (b) Rw::st(sp + n, 0);
      } else {
        Rw::add(S + n, a);
        if (b) Rw::add(sp + n, a * b);
      }
    }
  }
}

// sum over the entries p of the row [lo, hi) of S[cols[p]] = sum over m of A[t, m] (A A)[t, m] = K3[t, t]; this thread's share
template <bool kLds>
__device__ __forceinline__ long long ncn8_k3_part(const int32_t* __restrict__ cols, int lo, int hi, const int32_t* S) {
  long long s = 0;
  for (int p = lo + (int)threadIdx.x; p < hi; p += kNcn8Threads) s += Rows<kLds>::ld(S + cols[p]);
  return s;
}

template <bool kLds>
__global__ __launch_bounds__(kNcn8Threads) void ncn8_cn_kernel(Cn8Args a) {
  using Rw = Rows<kLds>;
  extern __shared__ int32_t s_rows[];
  __shared__ int s_id[kNcn8Threads];
  __shared__ float s_cf[5][kNcn8Threads];
  __shared__ double s_w[kNcn8Threads];
  __shared__ int s_cnt[kNcn8Waves];
  __shared__ long long s_k3[kNcn8Waves][2];
  const int tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
  const long long N = a.N;
  const int C = a.C;
  const float* __restrict__ x = a.x;
  const int32_t* __restrict__ cols = a.cols;
  int32_t* rows = kLds ? s_rows : a.ws + (long long)blockIdx.x * a.region;
  int32_t *Ri = rows, *Rj = rows + N, *Si = rows + 2 * N, *Sj = rows + 3 * N, *sp = rows + 4 * N;
  for (long long r = blockIdx.x; r < a.B; r += gridDim.x) {  // (r is the workgroup's: every barrier below is reached by all)
    const long long ti = ld_idx(a.tar, a.tar_is64, r), tj = ld_idx(a.tar, a.tar_is64, a.tar_stride + r);
    float* __restrict__ o = a.xs + r * a.ldxs;
    if (ti < 0 || ti >= N || tj < 0 || tj >= N) {  // a target outside the node table is not dereferenced: a zero row
      for (long long c = tid; c < a.ldxs; c += kNcn8Threads) o[c] = 0.f;
      continue;
    }
    const float* __restrict__ xi = x + ti * C;
    const float* __restrict__ xj = x + tj * C;
    for (int c = tid; c < C; c += kNcn8Threads) o[c] = xi[c] * xj[c];
    for (long long c = 8ll * C + tid; c < a.ldxs; c += kNcn8Threads) o[c] = 0.f;
    // every block is zero unless r is the last occurrence of both targets, each on its side
    const bool act = !a.last || (a.last[ti] == (int)r && a.last[N + tj] == (int)r);
    if (!act) {
      for (long long c = C + tid; c < 8ll * C; c += kNcn8Threads) o[c] = 0.f;
      continue;
    }
    const bool decay = a.last_update != nullptr;
    const long long et = decay ? (long long)a.edge_time[r] : 0;
    const int ilo = a.indptr[ti], ihi = a.indptr[ti + 1], jlo = a.indptr[tj], jhi = a.indptr[tj + 1];

    // ---- the count rows ----
    if (kLds) {
      for (long long t = tid; t < kNcn8Rows * N; t += kNcn8Threads) s_rows[t] = 0;
      __syncthreads();
    }
    ncn8_walk<kLds, false>(a.indptr, cols, ilo, ihi, jlo, jhi, Ri, Si, sp);
    ncn8_walk<kLds, false>(a.indptr, cols, jlo, jhi, 0, 0, Rj, Sj, nullptr);
    Rw::sync();

    // ---- K3[i, i], K3[j, j], u ----
    long long k3i = ncn8_k3_part<kLds>(cols, ilo, ihi, Si), k3j = ncn8_k3_part<kLds>(cols, jlo, jhi, Sj);
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      k3i += __shfl_down(k3i, off);
      k3j += __shfl_down(k3j, off);
    }
    if (lane == 0) s_k3[wave][0] = k3i, s_k3[wave][1] = k3j;
    __syncthreads();
    k3i = k3j = 0;
#pragma unroll
    for (int w = 0; w < kNcn8Waves; ++w) k3i += s_k3[w][0], k3j += s_k3[w][1];
    const int mij = count_in(cols, ilo, ihi, tj);  // A[i, j] = A[j, i]
    const long long u = -(long long)mij;

    // ---- c01, c10: one term each, as at k = 4 ----
    {
      const double w0 = mij ? (double)mij * (decay ? decay_weight_f64(a.last_update, et, ti) : 1.) : 0.;
      const double w1 = mij ? (double)mij * (decay ? decay_weight_f64(a.last_update, et, tj) : 1.) : 0.;
      for (int c = tid; c < C; c += kNcn8Threads) {
        o[C + c] = mij ? (float)(w0 * (double)xi[c]) : 0.f;
        o[2ll * C + c] = mij ? (float)(w1 * (double)xj[c]) : 0.f;
      }
    }

    // ---- the five sums: a pass per 256 channels, the ids 256 at a time ----
    for (int c0 = 0; c0 < C; c0 += kNcn8Threads) {
      const int c = c0 + tid;
      const bool mine = c < C;
      double acc[5] = {0., 0., 0., 0., 0.};
      for (long long n0 = 0; n0 < N; n0 += kNcn8Threads) {
        const long long n = n0 + tid;
        long long c11 = 0, c12 = 0, c21 = 0, c22 = 0, cs = 0;
        if (n < N) {
          const long long ri = Rw::ld(Ri + n), rj = Rw::ld(Rj + n), si = Rw::ld(Si + n), sj = Rw::ld(Sj + n);
          cs = Rw::ld(sp + n);
          c11 = ri * rj;
          if (n != ti && n != tj) {  // the column masks of c12, c21, c22
            c12 = ri * sj + ri * ri * u;
            c21 = si * rj + rj * rj * u;
            c22 = si * sj + ((ri > 0 ? k3i : 0) + (rj > 0 ? k3j : 0) - c11) * u + cs;
            if (c22 < 0) c22 = 0;
          }
        }
        const bool weighted = (c11 | c12 | c21 | c22) != 0;
        const bool any = weighted || cs != 0;
        const unsigned long long hits = __ballot(any);
        if (lane == 0) s_cnt[wave] = __popcll(hits);
        __syncthreads();
        int at = __popcll(hits & ((1ull << lane) - 1)), total = 0;
#pragma unroll
        for (int w = 0; w < kNcn8Waves; ++w) {
          if (w < wave) at += s_cnt[w];
          total += s_cnt[w];
        }
        if (any) {
          // W is applied only where a count is non-zero (the reference multiplies dense matrices: an infinite weight makes its zeros NaN)
          s_w[at] = decay && weighted ? decay_weight_f64(a.last_update, et, n) : 1.;
          s_id[at] = (int)n;
          s_cf[0][at] = (float)c11;
          s_cf[1][at] = (float)c12;
          s_cf[2][at] = (float)c21;
          s_cf[3][at] = (float)c22;
          s_cf[4][at] = (float)cs;  // special_2_2 carries no decay and no column mask
        }
        __syncthreads();
        if (mine) {
#pragma unroll 4
          for (int e = 0; e < total; ++e) {  // ascending ids
            const double xv = (double)x[(long long)s_id[e] * C + c];
            const double xw = s_w[e] * xv;
#pragma unroll
            for (int q = 0; q < 4; ++q) {  // (a zero count stays out even of an infinite weight)
              const float cf = s_cf[q][e];
              acc[q] = cf != 0.f ? __builtin_fma((double)cf, xw, acc[q]) : acc[q];
            }
            acc[4] = __builtin_fma((double)s_cf[4][e], xv, acc[4]);
          }
        }
        __syncthreads();  // the next chunk overwrites the list
      }
      if (mine) {
#pragma unroll
        for (int q = 0; q < 5; ++q) o[(3ll + q) * C + c] = (float)acc[q];
      }
    }

    if (!kLds) {  // leave the region zeroed for the next pair: the same walks, storing zeros
      ncn8_walk<kLds, true>(a.indptr, cols, ilo, ihi, jlo, jhi, Ri, Si, sp);
      ncn8_walk<kLds, true>(a.indptr, cols, jlo, jhi, 0, 0, Rj, Sj, nullptr);
      Rw::sync();
    }
  }
}

// The whole MLP of one pair in float64, h [H] kept in LDS unrounded (and written out as float32 for whoever reads the block's h): at k = 8 xs
// carries integer-weighted sums in the hundreds next to x[i] * x[j] of order 1, so the order of a float32 dot product over the 8 C inputs
// shows in the logits, and a hidden unit of 130 rounded to float32 carries 8e-6 into a logit of 3.6.  A workgroup per pair; a wave per
// hidden unit / output, the lanes over the dot product (coalesced), a butterfly in a fixed order: the same bits every run.
constexpr int kNcn8MlpMaxH = 8192;  // 64 KB of float64 hidden units, what a workgroup gets without opting in; a wider layer is refused
__global__ __launch_bounds__(kNcn8Threads) void ncn8_mlp_kernel(const float* __restrict__ xs, long long ldxs, const float* __restrict__ w1,
                                                                const float* __restrict__ b1, const float* __restrict__ w2,
                                                                const float* __restrict__ b2, float* __restrict__ h, long long ldh,
                                                                float* __restrict__ out, long long B, int H, int K, int O) {
  extern __shared__ double s_h[];
  const int lane = lane_id(), wave = threadIdx.x / kWave;
  for (long long r = blockIdx.x; r < B; r += gridDim.x) {
    const float* __restrict__ a = xs + r * ldxs;
    for (int j = wave; j < H; j += kNcn8Waves) {
      const float* __restrict__ w = w1 + (long long)j * K;
      double s = 0.;
#pragma unroll 4
      for (int k = lane; k < K; k += kWave) s = __builtin_fma((double)a[k], (double)w[k], s);
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_xor(s, off);
      s += (double)b1[j];
      s = s > 0. ? s : 0.;
      if (lane == 0) {
        s_h[j] = s;
        h[r * ldh + j] = (float)s;
      }
    }
    __syncthreads();
    for (int q = wave; q < O; q += kNcn8Waves) {
      const float* __restrict__ w = w2 + (long long)q * H;
      double s = 0.;
      for (int j = lane; j < H; j += kWave) s = __builtin_fma(s_h[j], (double)w[j], s);
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_xor(s, off);
      if (lane == 0) out[r * O + q] = (float)(s + (double)b2[q]);
    }
    __syncthreads();  // the next pair overwrites s_h
  }
}

static long long ncn8_groups(long long B) { return B < 1 ? 1 : (B > kNcn8MaxGroups ? kNcn8MaxGroups : B); }
static size_t ncn8_region_ints(long long N) { return ((size_t)kNcn8Rows * (size_t)N + 63) & ~(size_t)63; }

// > 64 KB of LDS per workgroup is a per-device opt-in of the kernel function
static bool ncn8_lds_optin() {
  constexpr int kMaxDevices = 64;
  static std::atomic<bool> done[kMaxDevices];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = -1;
  if (dev >= 0 && done[dev].load(std::memory_order_acquire)) return true;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ncn8_cn_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           kNcn8Rows * kNcn8LdsMaxN * (int)sizeof(int32_t));
  if (e != hipSuccess) {
    set_error("ncn8_cn_emb: cannot reserve LDS: %s", hipGetErrorString(e));
    return false;
  }
  if (dev >= 0) done[dev].store(true, std::memory_order_release);
  return true;
}

}  // namespace tgmx

using namespace tgmx;

extern "C" int32_t tgmx_ncn8_lds_max_nodes(void) { return kNcn8LdsMaxN; }

extern "C" size_t tgmx_ncn8_workspace_bytes(int64_t N, int64_t B) {
  if (N < 1 || N >= (1ll << 31) || B < 0 || B >= (1ll << 31)) return 0;
  if (N <= kNcn8LdsMaxN) return 256;  // the rows live in LDS
  WorkspaceCarver c(nullptr);
  c.take<int32_t>(ncn8_region_ints(N) * (size_t)ncn8_groups(B));
  return c.total();
}

extern "C" int tgmx_ncn8_cn_emb(const float* x, int64_t N, int32_t C, const int32_t* indptr, const int32_t* cols, const void* tar, int32_t tar_is64,
                                int64_t tar_stride, int64_t B, const int64_t* last_update, const int64_t* edge_time, int32_t* last, float* xs,
                                int64_t ldxs, void* workspace, size_t workspace_bytes, int32_t force_workspace, tgmx_stream_t stream) {
  TGMX_REQUIRE(C > 0 && N > 0 && N < (1ll << 31) && B >= 0 && B < (1ll << 31) && tar_stride >= B && ldxs >= 8ll * C,
               "ncn8_cn_emb: bad sizes C=%d N=%lld B=%lld ldxs=%lld", C, (long long)N, (long long)B, (long long)ldxs);
  if (B == 0) return TGMX_OK;
  TGMX_REQUIRE(x && indptr && cols && tar && xs, "ncn8_cn_emb: null pointer");
  TGMX_REQUIRE((last_update == nullptr) == (edge_time == nullptr), "ncn8_cn_emb: time decay needs last_update and edge_time");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (last && (rc = ncn_last_marks(tar, tar_is64, (long long)tar_stride, (long long)B, (long long)N, last, st))) return rc;
  Cn8Args a{x, (long long)N, C, indptr, cols, tar, tar_is64, (long long)tar_stride, (long long)B, last_update, edge_time, last, xs, (long long)ldxs,
            nullptr, 0};
  if (N <= kNcn8LdsMaxN && !force_workspace) {
    if (!ncn8_lds_optin()) return TGMX_E_LAUNCH;
    const size_t lds = (size_t)kNcn8Rows * (size_t)N * sizeof(int32_t);
    hipLaunchKernelGGL(ncn8_cn_kernel<true>, dim3(grid_for(B, 1, 16384)), dim3(kNcn8Threads), lds, st, a);
    TGMX_CHECK_LAUNCH("ncn8_cn_emb");
    return TGMX_OK;
  }
  const long long groups = ncn8_groups(B);
  WorkspaceCarver c(workspace);
  a.region = (long long)ncn8_region_ints(N);
  a.ws = c.take<int32_t>((size_t)a.region * (size_t)groups);
  if (!workspace || workspace_bytes < c.total()) {
    set_error("ncn8_cn_emb: workspace too small (%zu bytes, %zu needed)", workspace_bytes, c.total());
    return TGMX_E_INVALID;
  }
  if (hipMemsetAsync(a.ws, 0, (size_t)a.region * (size_t)groups * sizeof(int32_t), st) != hipSuccess) {  // once per call; the pairs clear behind them
    set_error("ncn8_cn_emb: clearing the workspace failed");
    return TGMX_E_LAUNCH;
  }
  hipLaunchKernelGGL(ncn8_cn_kernel<false>, dim3((unsigned)groups), dim3(kNcn8Threads), 0, st, a);
  TGMX_CHECK_LAUNCH("ncn8_cn_emb(workspace)");
  return TGMX_OK;
}

extern "C" int tgmx_ncn8_forward(const tgmx_ncn_fwd_t* a, void* workspace, size_t workspace_bytes, tgmx_stream_t stream) {
  TGMX_REQUIRE(a && a->k == 8 && a->H > 0 && a->out_ch > 0 && a->B >= 0 && a->C > 0, "ncn8_forward: bad argument block (k must be 8)");
  TGMX_REQUIRE(a->H <= kNcn8MlpMaxH, "ncn8_forward: hidden_dim %d is more than the %d the float64 MLP keeps in LDS", a->H, kNcn8MlpMaxH);
  TGMX_REQUIRE(a->ldxs % 4 == 0 && a->ldh % 4 == 0 && a->ldh >= a->H, "ncn8_forward: leading dimensions must be multiples of 4");
  int rc;
  if (!a->have_adj &&
      (rc = tgmx_ncn_adj_build(a->edge_index, a->ei_is64, a->ei_stride, a->E, a->N, a->indptr, a->cols, a->adj_ws, a->adj_ws_bytes, stream)))
    return rc;
  if (a->B == 0) return TGMX_OK;
  if ((rc = tgmx_ncn8_cn_emb(a->x, a->N, a->C, a->indptr, a->cols, a->tar, a->tar_is64, a->tar_stride, a->B, a->decay ? a->last_update : nullptr,
                             a->decay ? a->edge_time : nullptr, a->dup_all ? nullptr : a->last, a->xs, a->ldxs, workspace, workspace_bytes, 0, stream)))
    return rc;
  TGMX_REQUIRE(a->w1 && a->b1 && a->w2 && a->b2 && a->h && a->out, "ncn8_forward: null pointer");
  const int K = 8 * a->C;
  // (the reference's xs.relu() discards its result: negative entries reach the first Linear)
  hipLaunchKernelGGL(ncn8_mlp_kernel, dim3(grid_for(a->B, 1, 16384)), dim3(kNcn8Threads), (size_t)a->H * sizeof(double), (hipStream_t)stream, a->xs,
                     (long long)a->ldxs, a->w1, a->b1, a->w2, a->b2, a->h, (long long)a->ldh, a->out, (long long)a->B, a->H, K, a->out_ch);
  TGMX_CHECK_LAUNCH("ncn8_forward(mlp)");
  return TGMX_OK;
}
