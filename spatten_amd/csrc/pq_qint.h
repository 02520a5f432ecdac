// pq_qint.h — what the quantised-query decode kernels share (include/spatten.h "Quantised query"): the ONE device routine that
// quantises the rotated query — used by the per-query-head kernels (pq_decode.hip: both passes) and by the grouped MSB pass
// (pq_gqa.hip), whose refetch pass IS pq_decode.hip's: a different tie or a different last bit would pair an s1 scored with one
// q_int with an A2 scored with another — and the host-side hooks the grouped entry point needs from pq_decode.hip.
#pragma once
#include "common.h"

namespace spatten {

__device__ inline uint32_t pack_i8x4(int a, int b, int c, int d) {
  return (uint32_t)(a & 255) | ((uint32_t)(b & 255) << 8) | ((uint32_t)(c & 255) << 16) | ((uint32_t)(d & 255) << 24);
}

// q_scale = amax / qmax (one rounding); the divisor of an all-zero query is 1 (q_scale = 0, q_int = 0)
__device__ inline void qint_scale(float amax, float qmaxf, float& qs, float& qs_div) {
  qs = amax / qmaxf;
  qs_div = qs > 0.f ? qs : 1.0f;
}
// q_int = clamp(rint(x / q_scale)) with the quotient's last-bit error taken out through the exact residual (so the result is a
// nearest rounding of the TRUE quotient)
__device__ inline int qint_round(float x, float qs_div, float qmaxf) {
  float rq = rintf(x / qs_div);
  const float e = fmaf(-rq, qs_div, x);              // x - rq q_scale, one rounding
  rq += (e > 0.5f * qs_div) ? 1.f : (e < -0.5f * qs_div) ? -1.f : 0.f;
  return (int)fminf(fmaxf(rq, -qmaxf), qmaxf);
}

// the quantised-query extras of spatten_attn_decode_pq_qint (NULL: the query stays in the model dtype)
struct PqQintExtra { int8_t* q_int; int64_t qi_sb, qi_sh; float* q_scale; int qmax; };

// argument validation of the profiled step (pq_decode.hip): SPATTEN_OK and the device-side plane descriptor, or the error
int pq_validate(const spatten_pq_decode_args_t* a, PlanesDev& pd);
// ONLY the compact refetch pass of spatten_attn_decode_pq_qint (pq_decode.hip: the pass-2 instantiation, grid rows = flagged query
// heads, its own split layout) behind an MSB pass that left msb_logit, need_lsb and the unflagged heads' results; f16 / bf16
int pq_qint_refetch(const spatten_pq_decode_args_t* a, const PlanesDev& pd, const PqQintExtra& qx, hipStream_t st);

}  // namespace spatten
