// DensityOfStateEstimatorHook (the reference's examples/analytics/dos.py) for gfx950: the spectral density of one batch's graph by stochastic
// Chebyshev moments.  The reference builds a networkx graph, asks scipy for the normalised Laplacian, multiplies it 19 times into 100 random
// probe vectors in numpy and integrates a Chebyshev series -- milliseconds of Python around 1.5 MFLOP.  A batch-sized graph (<= 2 E nodes,
// <= 2 E stored entries, E <= 4096) fits LDS, so the whole recurrence runs out of LDS in one call of three launches:
//
//   dos_build_kernel    ONE workgroup.  2 E directed keys (row id << 32 | col id) sorted in LDS (bitonic, padded to a power of two), equal
//                       neighbours dropped (duplicates, reversed duplicates, and a self-loop's two keys collapse), row heads -> the sorted
//                       node ids, indptr and the degrees; every column's local index by binary search of the row-head ids.  Writes the CSR of
//                       S = L_norm - I (every stored entry -1 / sqrt(d_i d_j)) and a list of chunks for rows longer than kDosChunk.
//   dos_moments_kernel  grid = probe slices of PV columns.  CSR copied to LDS once; T_{m-1} and T_{m-2} are two [n, PV] LDS blocks; lanes run
//                       along the PV columns of a row, a wave covers 64 / PV rows.  T_m overwrites T_{m-2} in place (element (i, p) of
//                       T_{m-2} is read by its owner only), the block pointers swap: one barrier per moment (two when a row is chunked).
//                       Z is never stored: a sign is one counter_u32 call, kept as one bit per owned row in a 64-bit register mask.
//   dos_finish_kernel   ONE workgroup.  Column mean, Jackson factors, the sine series at n_pts points, diff and clip, all in double.
//
// Determinism: no float atomics anywhere.  A row's sum runs over its entries in CSR order, a chunked row's partial sums are added chunk by
// chunk, a moment's column sum goes thread (rows ascending) -> wave (xor tree) -> workgroup (waves ascending), the column mean is a fixed tree.
// Equal inputs give equal bits.
//
// Matrix instructions do not fit: a row holds two entries on average, there is no dense tile to feed an MFMA with.
//
// Past 4096 events the same estimate runs over a CSR in HBM: dos_large.hip.  dos_shared.h holds what the two routes share.
#include "dos_shared.h"

namespace tgmx {

constexpr int kDosMaxE = 4096;          // 2 E keys = 64 KB of LDS in the build kernel; n <= 8192 rows at PV = 1 in the moments kernel
constexpr int kDosBuildThreads = 1024;
constexpr int kDosBuildPer = 8;         // keys a build thread owns at most: pow2(2 kDosMaxE) / kDosBuildThreads
constexpr int kDosThreads = 512;        // moments kernel: 8 waves
constexpr int kDosWaves = kDosThreads / kWave;
// nnz <= 8192: at most 8192 / 65 = 126 rows are longer than kDosChunk, and their chunks number sum ceil(len / 64) <= 8192 / 64 + 126 = 254
constexpr int kDosMaxChunks = 256;
constexpr int kDosMaxSplit = 128;
constexpr unsigned long long kDosPadKey = ~0ull;  // sorts behind every key of ids < 2^31

// header words of the workspace
enum { kDosN = 0, kDosNnz = 1, kDosNChunks = 2, kDosNSplit = 3 };

struct DosArgs {
  const void* src;
  const void* dst;
  int E, src64, dst64;
  int P;  // key count padded to a power of two
  int nZ, nM, n_pts, PV;
  unsigned long long seed, call;
  int* head;      // [64]
  int* node_id;   // [2 E]
  int* indptr;    // [2 E + 1]
  int* cols;      // [2 E]
  float* vals;    // [2 E]
  int* chunks;    // [kDosMaxChunks][2]: begin, end
  int* split;     // [kDosMaxSplit][3]: row, first chunk, chunks
  double* cmom;   // [nM, nZ]
  double* cdf;    // [n_pts]
  double* dos;    // [n_pts - 1]
  unsigned long long* status;
};

// (dos_block_scan here: two counts packed as a << 16 | b in an unsigned; every total stays below 2^14)

// ---- (a) the batch's graph as the CSR of S ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kDosBuildThreads) void dos_build_kernel(DosArgs a) {
  extern __shared__ unsigned long long dos_keys[];  // [P + 1]; after the scan the same bytes hold s_nid [P] and s_ptr [P + 1]
  __shared__ unsigned s_wave[kDosBuildThreads / kWave];
  const int tid = threadIdx.x, P = a.P;
  unsigned long long* s_key = dos_keys;

  // the 2 E directed keys; an event with an endpoint outside [0, 2^31) is skipped (both its keys are padding) and flagged
  bool bad = false;
  for (int e = tid; e < P / 2; e += kDosBuildThreads) {
    unsigned long long k0 = kDosPadKey, k1 = kDosPadKey;
    if (e < a.E) {
      const long long s = ld_idx(a.src, a.src64, e), d = ld_idx(a.dst, a.dst64, e);
      if (s < 0 || d < 0 || s >= (1ll << 31) || d >= (1ll << 31)) bad = true;
      else k0 = ((unsigned long long)s << 32) | (unsigned long long)d, k1 = ((unsigned long long)d << 32) | (unsigned long long)s;
    }
    s_key[2 * e] = k0;
    s_key[2 * e + 1] = k1;
  }
  if (bad) atomicOr(a.status, (unsigned long long)TGMX_AN_BAD_ID);
  __syncthreads();

  // bitonic network over P keys, P / 2 compare-exchanges a step
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < P / 2; t += kDosBuildThreads) {
        const int i = 2 * t - (t & (j - 1)), l = i + j;
        const unsigned long long x = s_key[i], y = s_key[l];
        if ((x > y) == ((i & k) == 0)) s_key[i] = y, s_key[l] = x;
      }
      __syncthreads();
    }
  }

  // a thread owns `per` consecutive sorted keys: which are the first of their value (an entry), which the first of their row (a head)
  const int per = P >= kDosBuildThreads ? P / kDosBuildThreads : 1;
  const int first = tid * per;
  unsigned long long mine[kDosBuildPer];
  unsigned is_entry = 0, is_head = 0, cnt = 0;
#pragma unroll
  for (int q = 0; q < kDosBuildPer; ++q) {
    mine[q] = kDosPadKey;
    const int idx = first + q;
    if (q < per && idx < P) {
      const unsigned long long key = s_key[idx];
      mine[q] = key;
      if (key != kDosPadKey) {
        const unsigned long long prev = idx > 0 ? s_key[idx - 1] : kDosPadKey;
        const bool entry = idx == 0 || key != prev, head = idx == 0 || (key >> 32) != (prev >> 32);
        is_entry |= (unsigned)entry << q;
        is_head |= (unsigned)head << q;
        cnt += ((unsigned)entry << 16) + (unsigned)head;
      }
    }
  }
  unsigned total;
  const unsigned base = dos_block_scan(cnt, s_wave, &total);  // its barriers also end every read of s_key
  const int nnz = (int)(total >> 16), n = (int)(total & 0xFFFFu);
  int* s_nid = reinterpret_cast<int*>(dos_keys);
  int* s_ptr = s_nid + P;
  {
    int pos = (int)(base >> 16), row = (int)(base & 0xFFFFu);
#pragma unroll
    for (int q = 0; q < kDosBuildPer; ++q) {
      if ((is_head >> q) & 1u) {
        s_nid[row] = (int)(mine[q] >> 32);
        s_ptr[row] = pos;
        ++row;
      }
      pos += (is_entry >> q) & 1u;
    }
  }
  if (tid == 0) s_ptr[n] = nnz;
  __syncthreads();

  // every entry: its column's local index (every column id is a row id: the key set is symmetric) and its value.
  // vals = -1 / sqrt(d_i d_j) as ONE float expression: the degrees converted to float (exact, <= 8192), their float product (rounded once where it
  // needs more than 24 bits), IEEE sqrt, IEEE divide of -1 by it.  The product commutes: S_ij == S_ji.
  {
    int pos = (int)(base >> 16), row = (int)(base & 0xFFFFu) - 1;  // row of the key before this thread's first
#pragma unroll
    for (int q = 0; q < kDosBuildPer; ++q) {
      row += (is_head >> q) & 1u;
      if ((is_entry >> q) & 1u) {
        const int cid = (int)(mine[q] & 0xFFFFFFFFull);
        int lo = 0, hi = n;  // lower bound of cid in s_nid [0, n)
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_nid[mid] < cid) lo = mid + 1;
          else hi = mid;
        }
        const int j = lo < n ? lo : n - 1;
        const float di = (float)(s_ptr[row + 1] - s_ptr[row]), dj = (float)(s_ptr[j + 1] - s_ptr[j]);
        a.cols[pos] = j;
        a.vals[pos] = -1.f / __fsqrt_rn(di * dj);
        ++pos;
      }
    }
  }
  for (int r = tid; r <= n; r += kDosBuildThreads) {
    a.indptr[r] = s_ptr[r];
    if (r < n) a.node_id[r] = s_nid[r];
  }

  // the work list of long rows: a thread owns consecutive rows, so the list is in row order
  const int rper = (n + kDosBuildThreads - 1) / kDosBuildThreads;
  unsigned lcnt = 0;
  for (int r = tid * rper; r < min(n, (tid + 1) * rper); ++r) {
    const int len = s_ptr[r + 1] - s_ptr[r];
    if (len > kDosChunk) lcnt += (1u << 16) + (unsigned)((len + kDosChunk - 1) / kDosChunk);
  }
  unsigned ltotal;
  const unsigned lbase = dos_block_scan(lcnt, s_wave, &ltotal);
  int sp = (int)(lbase >> 16), ch = (int)(lbase & 0xFFFFu);
  for (int r = tid * rper; r < min(n, (tid + 1) * rper); ++r) {
    const int b = s_ptr[r], e = s_ptr[r + 1];
    if (e - b <= kDosChunk) continue;
    const int c = (e - b + kDosChunk - 1) / kDosChunk;
    if (sp < kDosMaxSplit && ch + c <= kDosMaxChunks) {  // always (the bounds above); a guard for the stores
      a.split[3 * sp] = r, a.split[3 * sp + 1] = ch, a.split[3 * sp + 2] = c;
      for (int q = 0; q < c; ++q) a.chunks[2 * (ch + q)] = b + q * kDosChunk, a.chunks[2 * (ch + q) + 1] = min(e, b + (q + 1) * kDosChunk);
    }
    ++sp;
    ch += c;
  }
  if (tid == 0) {
    a.head[kDosN] = n;
    a.head[kDosNnz] = nnz;
    a.head[kDosNChunks] = min((int)(ltotal & 0xFFFFu), kDosMaxChunks);
    a.head[kDosNSplit] = min((int)(ltotal >> 16), kDosMaxSplit);
  }
}

// ---- (b) the Chebyshev moments of a slice of probe columns -----------------------------------------------------------------------------

// LDS of one moments workgroup over at most nmax rows and nmax entries, PV columns wide (the host sizes it from 2 E: n is not read back)
__host__ __device__ inline size_t dos_lds_bytes(int nmax, int PV) {
  size_t b = 2 * (size_t)nmax * PV * sizeof(float);             // T_{m-1}, T_{m-2}
  b += (size_t)nmax * sizeof(float);                            // vals
  b += ((size_t)nmax + 2) * sizeof(int);                        // indptr (+ 1 to keep the doubles behind it 8-byte aligned)
  b += (size_t)kDosMaxChunks * 2 * sizeof(int) + (size_t)kDosMaxSplit * 4 * sizeof(int);
  b += (size_t)kDosMaxChunks * PV * sizeof(float);              // the chunks' partial sums
  b += 2 * (size_t)kDosWaves * PV * sizeof(double);             // the waves' column sums, two moments in flight
  b += ((size_t)nmax + 3) / 4 * 4 * sizeof(unsigned short);     // cols (n <= 8192 fits 16 bits)
  return b;
}
// the widest PV of {8, 4, 2, 1} that fits the budget with a 64-bit sign mask per thread (a thread owns <= 64 rows); 0: none
inline int dos_probe_width(long long E) {
  if (E < 1 || E > kDosMaxE) return 0;
  for (int pv = 8; pv >= 1; pv >>= 1)
    if (dos_lds_bytes((int)(2 * E), pv) <= kDosLdsBudget && 2 * E <= 64ll * (kDosThreads / pv)) return pv;
  return 0;
}

__device__ __forceinline__ float dos_sign(const DosArgs& a, int node, int col) { return dos_sign(a.seed, a.call, a.nZ, node, col); }

template <int PV>
__global__ __launch_bounds__(kDosThreads) void dos_moments_kernel(DosArgs a) {
  extern __shared__ double dos_lds[];
  const int n = a.head[kDosN], nnz = a.head[kDosNnz], nchunks = a.head[kDosNChunks], nsplit = a.head[kDosNSplit];
  const int nmax = 2 * a.E;
  double* s_cw = dos_lds;                                         // [2][kDosWaves][PV]
  float* s_t0 = reinterpret_cast<float*>(s_cw + 2 * kDosWaves * PV);
  float* s_t1 = s_t0 + (size_t)nmax * PV;
  float* s_val = s_t1 + (size_t)nmax * PV;
  float* s_part = s_val + nmax;                                   // [kDosMaxChunks][PV]
  int* s_ptr = reinterpret_cast<int*>(s_part + kDosMaxChunks * PV);  // [nmax + 2]
  int* s_chunk = s_ptr + nmax + 2;                                // [kDosMaxChunks][2]
  int* s_split = s_chunk + 2 * kDosMaxChunks;                     // [kDosMaxSplit][4]: row, first chunk, chunks, the row's node id
  unsigned short* s_col = reinterpret_cast<unsigned short*>(s_split + 4 * kDosMaxSplit);

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  constexpr int RP = kDosThreads / PV;  // rows a pass of the workgroup covers
  const int grp = tid / PV, p = tid % PV, col = blockIdx.x * PV + p;

  for (int i = tid; i <= n; i += kDosThreads) s_ptr[i] = a.indptr[i];
  for (int k = tid; k < nnz; k += kDosThreads) s_col[k] = (unsigned short)a.cols[k], s_val[k] = a.vals[k];
  for (int c = tid; c < 2 * nchunks; c += kDosThreads) s_chunk[c] = a.chunks[c];
  for (int k = tid; k < nsplit; k += kDosThreads) {
    const int r = a.split[3 * k];
    s_split[4 * k] = r, s_split[4 * k + 1] = a.split[3 * k + 1], s_split[4 * k + 2] = a.split[3 * k + 2], s_split[4 * k + 3] = a.node_id[r];
  }

  // T_0 = Z: the signs of this thread's rows (row grp + k RP is bit k), kept for the moments' Z . T_m
  unsigned long long neg = 0;
  double dsum = 0.0;
  {
    int k = 0;
    for (int i = grp; i < n; i += RP, ++k) {
      const float z = dos_sign(a, a.node_id[i], col);
      if (z < 0.f) neg |= 1ull << k;
      s_t0[i * PV + p] = z;
      dsum += 1.0;
    }
  }
  float* cur = s_t0;  // T_{m-1}
  float* old = s_t1;  // T_{m-2}, overwritten by T_m

  for (int m = 0; m < a.nM; ++m) {
    if (m > 0) {  // behind the barrier that ended moment m - 1: T_{m-1} is complete (m = 1: and the CSR is in LDS)
      dsum = 0.0;
      int k = 0;
      for (int i = grp; i < n; i += RP, ++k) {
        const int b = s_ptr[i], e = s_ptr[i + 1];
        if (e - b > kDosChunk) continue;  // a chunked row: below
        float acc = 0.f;
        for (int q = b; q < e; ++q) acc = __fmaf_rn(s_val[q], cur[(int)s_col[q] * PV + p], acc);
        const float t = m == 1 ? acc : __fmaf_rn(2.f, acc, -old[i * PV + p]);
        old[i * PV + p] = t;
        dsum += (double)(((neg >> k) & 1ull) ? -t : t);
      }
      if (nsplit > 0) {  // uniform over the workgroup
        for (int c = grp; c < nchunks; c += RP) {
          float acc = 0.f;
          for (int q = s_chunk[2 * c]; q < s_chunk[2 * c + 1]; ++q) acc = __fmaf_rn(s_val[q], cur[(int)s_col[q] * PV + p], acc);
          s_part[c * PV + p] = acc;
        }
        __syncthreads();
        for (int s = grp; s < nsplit; s += RP) {
          const int i = s_split[4 * s], c0 = s_split[4 * s + 1], cn = s_split[4 * s + 2];
          float acc = 0.f;
          for (int c = c0; c < c0 + cn; ++c) acc += s_part[c * PV + p];  // chunk by chunk, in row order
          const float t = m == 1 ? acc : __fmaf_rn(2.f, acc, -old[i * PV + p]);
          old[i * PV + p] = t;
          dsum += (double)(t * dos_sign(a, s_split[4 * s + 3], col));
        }
      }
      float* const sw = cur;
      cur = old;
      old = sw;
    }
    // c[m, col] = sum over the rows: the lanes of a wave that share p (xor tree), then the waves in order
#pragma unroll
    for (int off = PV; off < kWave; off <<= 1) dsum += __shfl_xor(dsum, off);
    double* cw = s_cw + (m & 1) * kDosWaves * PV;
    if (lane < PV) cw[wave * PV + lane] = dsum;
    __syncthreads();  // the moment's one barrier.  Moment m + 2 writes cw again only behind the barrier of m + 1, which wave 0 reaches after its read
    if (tid < PV && col < a.nZ) {
      double c = 0.0;
#pragma unroll
      for (int w = 0; w < kDosWaves; ++w) c += cw[w * PV + tid];
      a.cmom[(size_t)m * a.nZ + col] = c;
    }
  }
}

// ---- (c) mean, Jackson filter, Chebyshev integration, diff and clip: dos_finish_kernel (dos_shared.h) ------------------------------------

static int dos_pow2(long long v) {
  int p = 2;
  while (p < v) p <<= 1;
  return p;
}
static size_t dos_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace tgmx

using namespace tgmx;

extern "C" int32_t tgmx_dos_supported(int64_t E, int32_t nZ, int32_t nM, int32_t n_pts) {
  return E >= 1 && E <= kDosMaxE && nZ >= 1 && nZ <= 1024 && nM >= 2 && nM <= 64 && n_pts >= 2 && n_pts <= 65536 && dos_probe_width(E) > 0;
}

extern "C" int32_t tgmx_dos_probe_width(int64_t E) { return dos_probe_width(E); }

extern "C" size_t tgmx_dos_workspace_bytes(int64_t E, int32_t nZ, int32_t nM, int32_t n_pts) {
  if (!tgmx_dos_supported(E, nZ, nM, n_pts)) return 0;
  const size_t n2 = 2 * (size_t)E;
  return 256 + dos_align(64 * sizeof(int)) + 3 * dos_align(n2 * sizeof(int)) + dos_align((n2 + 1) * sizeof(int)) +
         dos_align(kDosMaxChunks * 2 * sizeof(int)) + dos_align(kDosMaxSplit * 3 * sizeof(int)) + dos_align((size_t)nM * nZ * sizeof(double)) +
         dos_align((size_t)n_pts * sizeof(double));
}

extern "C" int tgmx_dos_estimate(const tgmx_dos_t* args, tgmx_stream_t stream) {
  TGMX_REQUIRE(args, "dos_estimate: null pointer");
  const tgmx_dos_t& t = *args;
  TGMX_REQUIRE(tgmx_dos_supported(t.E, t.nZ, t.nM, t.n_pts), "dos_estimate: outside the envelope (E=%lld nZ=%d nM=%d n_pts=%d)", (long long)t.E, t.nZ,
               t.nM, t.n_pts);
  TGMX_REQUIRE(t.src && t.dst && t.dos && t.status && t.workspace, "dos_estimate: null pointer");
  const size_t need = tgmx_dos_workspace_bytes(t.E, t.nZ, t.nM, t.n_pts);
  TGMX_REQUIRE(t.workspace_bytes >= need, "dos_estimate: workspace too small (%zu of %zu bytes)", t.workspace_bytes, need);
  DosArgs a{};
  a.src = t.src, a.dst = t.dst, a.E = (int)t.E, a.src64 = t.src_is64 != 0, a.dst64 = t.dst_is64 != 0;
  a.P = dos_pow2(2 * t.E);
  a.nZ = t.nZ, a.nM = t.nM, a.n_pts = t.n_pts, a.PV = dos_probe_width(t.E);
  a.seed = t.seed, a.call = t.call;
  const size_t n2 = 2 * (size_t)t.E;
  char* w = reinterpret_cast<char*>(((uintptr_t)t.workspace + 255) & ~(uintptr_t)255);
  auto take = [&w](size_t bytes) {
    char* p = w;
    w += dos_align(bytes);
    return p;
  };
  a.head = reinterpret_cast<int*>(take(64 * sizeof(int)));
  a.node_id = reinterpret_cast<int*>(take(n2 * sizeof(int)));
  a.cols = reinterpret_cast<int*>(take(n2 * sizeof(int)));
  a.vals = reinterpret_cast<float*>(take(n2 * sizeof(float)));
  a.indptr = reinterpret_cast<int*>(take((n2 + 1) * sizeof(int)));
  a.chunks = reinterpret_cast<int*>(take(kDosMaxChunks * 2 * sizeof(int)));
  a.split = reinterpret_cast<int*>(take(kDosMaxSplit * 3 * sizeof(int)));
  a.cmom = reinterpret_cast<double*>(take((size_t)t.nM * t.nZ * sizeof(double)));
  a.cdf = reinterpret_cast<double*>(take((size_t)t.n_pts * sizeof(double)));
  a.dos = t.dos;
  a.status = reinterpret_cast<unsigned long long*>(t.status);
  hipStream_t st = (hipStream_t)stream;

  const size_t build_lds = ((size_t)a.P + 1) * sizeof(unsigned long long);
  static std::atomic<bool> build_attr[64];
  if (build_lds > 64 * 1024 && !dos_reserve_lds(dos_build_kernel, build_attr, ((size_t)dos_pow2(2 * kDosMaxE) + 1) * sizeof(unsigned long long)))
    return TGMX_E_LAUNCH;
  hipLaunchKernelGGL(dos_build_kernel, dim3(1), dim3(kDosBuildThreads), build_lds, st, a);
  TGMX_CHECK_LAUNCH("dos_estimate(build)");

  const size_t lds = dos_lds_bytes((int)n2, a.PV);
  const dim3 grid((unsigned)((t.nZ + a.PV - 1) / a.PV));
  static std::atomic<bool> mom_attr[4][64];
#define TGMX_DOS_MOMENTS(pv, slot)                                                                                  \
  do {                                                                                                              \
    if (lds > 64 * 1024 && !dos_reserve_lds(dos_moments_kernel<pv>, mom_attr[slot], kDosLdsBudget)) return TGMX_E_LAUNCH; \
    hipLaunchKernelGGL(dos_moments_kernel<pv>, grid, dim3(kDosThreads), lds, st, a);                                \
  } while (0)
  switch (a.PV) {
    case 8: TGMX_DOS_MOMENTS(8, 0); break;
    case 4: TGMX_DOS_MOMENTS(4, 1); break;
    case 2: TGMX_DOS_MOMENTS(2, 2); break;
    default: TGMX_DOS_MOMENTS(1, 3); break;
  }
#undef TGMX_DOS_MOMENTS
  TGMX_CHECK_LAUNCH("dos_estimate(moments)");

  hipLaunchKernelGGL(dos_finish_kernel<DosArgs>, dim3(1), dim3(kDosFinishThreads), 0, st, a);
  TGMX_CHECK_LAUNCH("dos_estimate(finish)");
  return TGMX_OK;
}
