// Device pieces that several sources share: the MFMA accumulator types and the operand loader of the GEMM (csrc/dense.hip, csrc/tgat.hip).
#pragma once
#include "common.h"

namespace tgmx {

using floatx16 = __attribute__((__vector_size__(16 * sizeof(float)))) float;  // accumulator of v_mfma_f32_32x32x2_f32
using floatx4 = __attribute__((__vector_size__(4 * sizeof(float)))) float;    // accumulator of the 16 x 16 MFMAs

// kGemmK consecutive k of a row from kb on: 16-byte loads where VEC (aligned row) and inside K, else float by float, zeros past K
template <bool VEC, int kGemmK>
__device__ __forceinline__ void load_kn(const float* __restrict__ row, int kb, int K, float (&v)[kGemmK]) {
#pragma unroll
  for (int c = 0; c < kGemmK; c += 4) {
    if (VEC && kb + c + 4 <= K) {
      const float4 x = *reinterpret_cast<const float4*>(row + kb + c);
      v[c] = x.x; v[c + 1] = x.y; v[c + 2] = x.z; v[c + 3] = x.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) v[c + u] = kb + c + u < K ? row[kb + c + u] : 0.f;
    }
  }
}

}  // namespace tgmx
