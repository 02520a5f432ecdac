// prune_rows.h — device code shared by the prune events: prune.hip (one length for the whole batch, host integers) and
// prune_ragged.hip (one length per sequence, read on the device): the parameter block and helpers of the window top-k with the window in registers
// (its body: select_reg_body.inc; the rotated shadow of a moved row: rope_piece_pair.inc).
#pragma once
#include "common.h"

namespace spatten {

// window top-k -> ascending absolute positions: what a select kernel is told
template <typename T>
struct SelectParams {
  const T* score;                 // single-layer base, or
  const void* const* score_ptrs;  // per-layer pointers (device memory)
  int64_t score_sh;
  int32_t* idx;                   // [layers, H, k] via idx_sl, idx_sh
  int64_t idx_sl, idx_sh;
  int H, lo, hi, k;
};

// The same selection with the whole window in REGISTERS (windows up to 32768 scores): one workgroup of NT threads per
// (layer, head) — workgroup `blk` of layers * H serves head blk % H of layer blk / H, VPT consecutive scores per thread, read once.  The k-th largest key is found two bits at a time: per
// pass every key is classed 0..3 against the prefix found so far (saturating subtract, shift, min) and counted in a
// byte field of one register — five VALU operations per key, no shuffles and no same-address LDS atomics (real score
// windows concentrate in a handful of exponent bins, which serialises a histogram) — then one DPP wave reduction and
// two LDS adds per wave.  The compaction is ONE packed (greater, equal) block scan.  Same result as
// topk_select_kernel bit for bit (same keys, same tie rule).  The body is select_reg_body.inc; these are its helpers.
template <int CTRL>
__device__ inline unsigned dpp_u32(unsigned x) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true);
}
__device__ inline unsigned wave_sum_u32(unsigned v) {
  v += dpp_u32<kDppXor1>(v);
  v += dpp_u32<kDppXor2>(v);
  v += dpp_u32<kDppHalfMirror>(v);
  v += dpp_u32<kDppMirror>(v);
  auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = r[0] + r[1];
  r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return r[0] + r[1];
}

}  // namespace spatten
