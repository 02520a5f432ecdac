// select_row.h — the k largest of one score row as ascending positions (radix select on the order-preserving key + an
// order-preserving compaction; ties at the k-th value: lowest index first, TopK.scala:193-212).  One workgroup of kSelThreads
// threads per row.  Shared by prune.hip (the window top-k of the prune event) and pq_decode.hip (the kept rows of local V pruning
// over the quantised planes).
#pragma once
#include "common.h"

namespace spatten {

constexpr int kSelThreads = 256;

// row [W] (contiguous), 0 < k <= W: out[0..k) = lo + the kept positions, ascending
template <typename T>
__device__ inline void topk_select_row(const T* row, int W, int k, int lo, int32_t* out) {
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_sel[2];          // digit, count strictly above it
  __shared__ unsigned s_cnt[2][4][2];    // [parity][wave][gt, eq]

  const int tid = threadIdx.x;
  const int lane = tid % kWave;
  const int wave = tid / kWave;

  // ---- radix select: the key of the k-th largest element ----------------------------------------
  // fp32 keys of bf16 values populate the top 16 bits, of f16 values the top 19 (1+8+10), fp32 all 32.
  // The radix passes only look at those bits, so the key is masked to them everywhere (the all-ones NaN key
  // would otherwise compare GREATER than the threshold assembled from the passes and over-fill the output).
  constexpr int kPasses = sizeof(T) == 4 ? 4 : (DT<T>::kId == SPATTEN_BF16 ? 2 : 3);
  constexpr unsigned kKeyMask = kPasses == 4 ? 0xFFFFFFFFu : (kPasses == 3 ? 0xFFFFFF00u : 0xFFFF0000u);
  unsigned prefix = 0, pmask = 0;
  unsigned k_rem = (unsigned)k;
#pragma unroll 1
  for (int pass = 0; pass < kPasses; ++pass) {
    const int shift = 24 - 8 * pass;
    s_hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < W; i += kSelThreads) {
      const unsigned key = ordered_key(DT<T>::to_f32(row[i])) & kKeyMask;
      if ((key & pmask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (wave == 0) {
      // lane l owns the 4 bins 255-4l .. 252-4l (descending); inclusive scan over lanes
      unsigned c[4], tot = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { c[j] = s_hist[255 - 4 * lane - j]; tot += c[j]; }
      unsigned inc = tot;
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) {
        const unsigned t = __shfl_up(inc, off, kWave);
        if (lane >= off) inc += t;
      }
      unsigned ex = inc - tot;
      if (ex < k_rem && k_rem <= inc) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (ex < k_rem && k_rem <= ex + c[j]) { s_sel[0] = 255 - 4 * lane - j; s_sel[1] = ex; }
          ex += c[j];
        }
      }
    }
    __syncthreads();
    prefix |= s_sel[0] << shift;
    pmask |= 255u << shift;
    k_rem -= s_sel[1];
  }
  const unsigned thr = prefix;       // key of the k-th largest
  const unsigned need_eq = k_rem;    // how many elements equal to it are kept (>= 1), lowest index first

  // ---- order-preserving compaction --------------------------------------------------------------
  unsigned run_eq = 0, run_kept = 0;
  int parity = 0;
  for (int base = 0; base < W; base += kSelThreads, parity ^= 1) {
    const int i = base + tid;
    unsigned key = 0;
    const bool in = i < W;
    if (in) key = ordered_key(DT<T>::to_f32(row[i])) & kKeyMask;
    const bool gt = in && key > thr;
    const bool eq = in && key == thr;
    const unsigned long long m_gt = __ballot(gt);
    const unsigned long long m_eq = __ballot(eq);
    if (lane == 0) { s_cnt[parity][wave][0] = __popcll(m_gt); s_cnt[parity][wave][1] = __popcll(m_eq); }
    __syncthreads();
    unsigned eq_base = run_eq, kept_base = run_kept;
    unsigned tot_eq = run_eq, tot_kept = run_kept;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const unsigned g = s_cnt[parity][w][0], e = s_cnt[parity][w][1];
      const unsigned room = tot_eq < need_eq ? need_eq - tot_eq : 0u;
      const unsigned kept_w = g + (e < room ? e : room);
      if (w < wave) { eq_base += e; kept_base += kept_w; }
      tot_eq += e;
      tot_kept += kept_w;
    }
    const unsigned long long lt = (1ull << lane) - 1ull;
    const unsigned my_eq_rank = eq_base + __popcll(m_eq & lt);
    const bool keep = gt || (eq && my_eq_rank < need_eq);
    const unsigned long long m_keep = __ballot(keep);
    const unsigned pos = kept_base + __popcll(m_keep & lt);
    if (keep && pos < (unsigned)k) out[pos] = lo + i;      // pos < k always holds; the guard keeps a logic slip local
    run_eq = tot_eq;
    run_kept = tot_kept;
  }
}

}  // namespace spatten
