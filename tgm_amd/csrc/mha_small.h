// What tgmx_mha_small (csrc/dygformer.hip) and its backward (csrc/dygformer_bwd.hip) share: the envelope's constants and the LDS pitches.
#pragma once
#include <stddef.h>

namespace tgmx {

constexpr int kMhaMaxT = 128;         // tokens per pair
constexpr int kMhaMaxDh = 128;        // head dimension
constexpr int kMhaJ = kMhaMaxT / 16;  // score tiles per row tile
constexpr size_t kMhaMaxLds = 160 * 1024;

inline int mha_ld(int n4) { return (n4 / 4) % 2 ? n4 : n4 + 4; }  // multiple of 4, 4 (mod 8)

// The backward's pitches for its two T x T tiles (ds_read_b32: 32 banks, conflicts counted within a 32-lane half = two of the four
// 4-lane k groups).  An operand read as rows (address (16 i + lc) ld + k + lg) wants ld = 2 (mod 4); read transposed
// (address (k + lg) ld + 16 i + lc) it wants ld = 16 (mod 32).  The dropped probabilities are only read transposed: 16 (mod 32).
// dS is read both ways: 18 (mod 32) -- rows conflict-free, transposed two banks of a half met twice.
inline int mha_bwd_ld_pm(int Tp) { return (Tp + 15) / 32 * 32 + 16; }
inline int mha_bwd_ld_ds(int Tp) { return (Tp + 13) / 32 * 32 + 18; }

// LDS of one workgroup of the backward: Q, K, V, dO [Tp, ldk] and the two T x T tiles, all resident
inline size_t mha_bwd_lds_bytes(int T, int dh) {
  const int Tp = (T + 15) & ~15, ldk = mha_ld((dh + 3) & ~3);
  return sizeof(float) * (size_t)Tp * (4 * (size_t)ldk + mha_bwd_ld_pm(Tp) + mha_bwd_ld_ds(Tp));
}

}  // namespace tgmx
