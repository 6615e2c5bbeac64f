// What the two routes of DensityOfStateEstimatorHook share (dos.hip: the batch's graph in LDS, E <= 4096; dos_large.hip: the graph as a CSR
// in HBM, E <= 2^22): the probe sign, the workgroup scan of packed counts, the finish kernel and the > 64 KB LDS opt-in.
#pragma once
#include <atomic>

#include "common.h"

namespace tgmx {

constexpr int kDosChunk = 64;           // a row longer than this is summed in chunks of this many entries
constexpr size_t kDosLdsBudget = 160 * 1024;  // gfx950's LDS per CU; one workgroup may take all of it
constexpr int kDosFinishThreads = 1024;

// Z[node, col]: +1 if bit 31 of counter_u32(seed, call, node * nZ + col) is clear, else -1
__device__ __forceinline__ float dos_sign(unsigned long long seed, unsigned long long call, int nZ, int node, int col) {
  return (counter_u32(seed, call, (unsigned long long)(unsigned)node * (unsigned long long)nZ + (unsigned long long)col) >> 31) ? -1.f : 1.f;
}

// Exclusive scan over the workgroup (a multiple of 64 threads, <= 1024) of two counts packed into one T as a << (bits of T / 2) | b; the
// caller keeps every total below half of T's bits, so the halves never carry into each other.  *total: the sum over all threads.
template <typename T>
__device__ __forceinline__ T dos_block_scan(T v, T* s_wave, T* total) {
  const int lane = lane_id(), wave = threadIdx.x / kWave, waves = blockDim.x / kWave;
  T incl = v;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const T o = __shfl_up(incl, off);
    if (lane >= off) incl += o;
  }
  if (lane == kWave - 1) s_wave[wave] = incl;
  __syncthreads();
  T before = 0, all = 0;
  for (int w = 0; w < waves; ++w) {
    const T t = s_wave[w];
    if (w < wave) before += t;
    all += t;
  }
  __syncthreads();  // s_wave may be written again
  *total = all;
  return before + incl - v;
}

// ---- mean, Jackson filter, Chebyshev integration, diff and clip: ONE workgroup, all in double.  Args: nM, nZ, n_pts, cmom [nM, nZ],
// cdf [n_pts] scratch, dos [n_pts - 1] ----------------------------------------------------------------------------------------------------

template <typename Args>
__global__ __launch_bounds__(kDosFinishThreads) void dos_finish_kernel(Args a) {
  __shared__ double s_c[64];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int nM = a.nM, nZ = a.nZ, n_pts = a.n_pts;
  const double pi = 3.14159265358979323846;
  // c_m = the mean over the columns: lane l adds columns l, l + 64, ... in order, then an xor tree; times the Jackson factor
  for (int m = wave; m < nM; m += kDosFinishThreads / kWave) {
    double s = 0.0;
    for (int j = lane; j < nZ; j += kWave) s += a.cmom[(size_t)m * nZ + j];
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) s += __shfl_xor(s, off);
    if (lane == 0) {
      const double N = (double)nM, tau = pi / (N + 1.0);
      const double g = ((N - m + 1.0) * cos(tau * m) + sin(tau * m) / tan(tau)) / (N + 1.0);
      s_c[m] = g * (s / (double)nZ);
    }
  }
  __syncthreads();
  // cdf at x_i of linspace(-1 + 1e-8, 1 - 1e-8, n_pts) (numpy's: start + i step, the last point the stop itself)
  const double lo = -1.0 + 1e-8, hi = 1.0 - 1e-8, step = (hi - lo) / (double)(n_pts - 1);
  for (int i = tid; i < n_pts; i += kDosFinishThreads) {
    const double x = i == n_pts - 1 ? hi : lo + (double)i * step;
    const double th = acos(x);
    double y = s_c[0] * (th - pi) / 2.0;
    for (int m = 1; m < nM; ++m) y += s_c[m] * sin((double)m * th) / (double)m;
    a.cdf[i] = y * (-2.0 / pi);
  }
  __syncthreads();  // the workgroup's own stores to cdf are visible to it
  for (int i = tid; i < n_pts - 1; i += kDosFinishThreads) {
    const double d = a.cdf[i + 1] - a.cdf[i];
    a.dos[i] = d > 0.0 ? d : 0.0;
  }
}

// > 64 KB of dynamic LDS is a per-device opt-in of the function (as tgat.hip's chain kernel), made once for `bytes`: the most the function
// ever asks for (its static LDS counts against the 160 KB too)
template <typename K>
static bool dos_reserve_lds(K kernel, std::atomic<bool>* flags, size_t bytes) {
  constexpr int kMaxDevices = 64;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = -1;
  if (dev >= 0 && flags[dev].load(std::memory_order_acquire)) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
    (void)hipGetLastError();
    set_error("dos_estimate: cannot reserve %zu bytes of LDS", bytes);
    return false;
  }
  if (dev >= 0) flags[dev].store(true, std::memory_order_release);
  return true;
}

}  // namespace tgmx
