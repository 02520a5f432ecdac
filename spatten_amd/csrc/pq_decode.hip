// pq_decode.hip — the decode step over PROFILED quantised planes (ABI 4): key MSB plane of 4 / 6 / 8 bits + 4-bit LSB plane,
// value plane of 8 / 6 bits (include/spatten.h "Bit profiles and the quantised VALUE plane").  PARITY UNPINNED: the
// reference's Python has no numeric implementation; restated from the RTL and checked against oracle/spatten_oracle.py.
//
//   MatrixFetcher.scala:48-51        supported (bit_count, fused_mat) profiles (4,1) (6,2) (8,1)
//   TestSpAtten.scala:64,83-97,173-176   the harness fetches K at quant_key_bit and V at quant_value_bit (8 by default, 6 in the
//                                    per8 trace); SpAttenController.scala:716-723: V is ONE fetch (`high_bits := True`)
//   SpAttenController.scala:35-39,230-232,296-305   the refetch adds 4 LSBs from a separate plane (write mask 0x00F)
//   RequantDecision.scala:44-72      need_requant = max_j prob_j < threshold;  SpAttenController.scala:402: recompute ONCE
//
// Two launches per step (same grid): PASS 1 scores every key from the MSB plane (logit = 16 (q . msb) scale / sqrt(d), fp32),
// leaves the fp32 MSB logits in planes.msb_logit, runs softmax + P.V over the quantised V and records need_lsb per head in the
// merge step; PASS 2 does work only for the flagged heads: it reads the stashed MSB logit + the LSB plane — logit8 = logit_msb
// + (q . lsb) scale / sqrt(d), the MSB plane is NOT re-read — and streams V again (the probabilities changed).
// HBM bytes per key row, d = 128: profile (4, 8): 64 + 128 + 8 (+ 4 written) in pass 1 and 4 + 64 + 128 + 8 in pass 2,
// against 64 + 256 + 4 and 128 + 256 + 4 with bf16 V (decode_attn.hip KSRC 1 / 2); (8, 8): 128 + 128 + 8; (6, 6): 96 + 96 + 8.
//
// Structure = the pipelined instantiation of decode_attn.hip's decode_body (split-N over one workgroup per CU, per-thread
// online softmax, tiles of UP row-groups double buffered, every load of a tile unconditional and issued before the previous
// tile is processed, the same publish / poll merge of the split partials on the SAME workspace protocol); the launch appends
// nothing (spatten_kv_append[_step] + spatten_pq_pack_planes first).  DYN = the device-resident length (step.hip).
// Every plane is in PIECE order (lane c of a row's D/16 lanes owns 16 elements = its piece): a lane's key piece, value piece
// and query elements line up, so there is no cross-lane traffic before the D/16-lane reduction of the logit.  Loads are
// 32-bit-offset buffer loads; the loop carries no branches per row-group.  r04 first cut (natural-layout nibble plane,
// flat loads with clamped rows, per-row-group branches, IEEE divide per logit): 3,000 instructions per 16 row-groups and
// 19.1 us per launch at 8192 rows x 32 heads — issue-bound, not byte-bound (2.8 TB/s).
#include <stdlib.h>

#include <algorithm>
#include <cmath>

#include "common.h"
#include "pq_pack.h"
#include "pq_qint.h"
#include "select_row.h"

namespace spatten {

template <typename T>
struct PqvParams {
  const T* q; int64_t q_sb, q_sh;
  PlanesDev pl;
  const T* cos; const T* sin; int table_rows;
  int step_sb;                                   // bytes between the states of consecutive sequences (RG; in the block's former padding)
  T* out; int64_t out_sb;
  T* scores; int64_t sc_sb, sc_sh;
  float* lse;
  const int32_t* head_ids;
  float thr; int32_t* need; float* head_abs; const int32_t* step;
  unsigned long long* ws_part; unsigned* ws_cnt; unsigned* ws_err; int64_t ws_unit;
  int B, H, Hkv, N, pos_q, S, chunk, poll_merge;
  float sqrt_d;
  // the step's APPEND inside the MSB pass (round 5, optional): row N - 1 of kc (optional) / krc / vc <- k_new / v_new [B,Hkv,d]
  // (modify_llama.py:95-104; the key rotated with rotary row nr_row of cos / sin) and that row of every plane
  const T* k_new; const T* v_new; int64_t new_sb, new_sh; T* kc; T* krc; T* vc; int64_t kv_sb, kv_sh; int nr_row;
  // the refetch pass over the FLAGGED heads only (round 6): blockIdx.y = rank among the flagged heads of the launch's n_act heads
  // (every workgroup derives the list itself from `need`: one wave load + ballot, no counter to reset), S / chunk of this pass are
  // its own — many short splits, so that two or three flagged heads are spread over the chip instead of over 8 CUs each
  int compact, n_act, S1, chunk1;                // (S1 / chunk1: pass 1's layout, taken when most heads are flagged)
  // the SCORES-ONLY form (SO: local V pruning over the planes, spatten_attn_decode_pq_local_v): the MSB pass folds the previous
  // step's probabilities into acc[h, j] (j < prev_len; DYN: state word 3) from the fp32 logits that step left in msb_logit and its
  // (max, sum) in prev_lse — read before this pass overwrites the row, by the thread that overwrites it
  // the CASCADE form of the full step (CF, spatten_attn_decode_pq_cascade): the same fold inside the full MSB pass; the refetch pass
  // writes the flagged heads' final logits back to msb_logit, and the merging workgroup of either pass publishes the unit's (max, sum)
  // to prev_lse (the kernel comment carries the ordering argument)
  // the RAGGED cascade form (CF && RG, spatten_attn_decode_pq_cascade_ragged): acc_sb = ELEMENTS between the accumulators of
  // consecutive sequences — 32 bits in the block's padding behind prev_len, like step_sb: the block keeps its size and every field
  // its offset, so every older instantiation keeps its code down to the offsets of the hidden arguments behind the block
  float* acc; int64_t acc_sh; float* prev_lse; int prev_len; int acc_sb;
  // the QUANTISED QUERY form (QI, spatten_attn_decode_pq_qint): the rotated query quantised once per head to qmax = 2^(query_bits-1) - 1
  // levels, every key scored with integer dot products; split 0 of the MSB pass exports q_int [B,H,d] (element order) and q_scale [B,H]
  int8_t* qi_out; int64_t qi_sb, qi_sh; float* qs_out; int qmax;
};

// row-groups per pipelined tile.  r04 A/B at 8192 rows x 32 heads, profile (4, 8), MSB pass: 12: 20.0 us, 8: 16.6, 6: 16.4, 4: 14.8
constexpr int kPqvUp = 4;
// (r04, 8192 rows x 32 heads, MSB pass of the (4,8) / (8,8) / (6,6) profiles: 256 threads 14.9 / 17.3 / 16.0 us; 512 (two waves per
//  SIMD, decode_attn.hip's 512-thread team) with 4 row-groups 16.9 / 18.2 / 18.3, with 2: 15.3 / 16.8 / 16.8 — the pipelined stream does
//  not gain from the second wave)
// (r05, measured and dropped: THREE tiles in flight instead of two — (4,8) 14.5 -> 15.3-15.5 us, (8,8) 16.9 -> 18.0-18.2, with tiles of
//  64 rows 14.7 / 17.7-18.1: the pass is not waiting for bytes in flight)
constexpr int kPqvThreads = 256;
constexpr int kPqvWaves = kPqvThreads / 64;

__device__ inline void pqv_store_granule(unsigned long long* g, float v, unsigned tag) {
  __hip_atomic_store(g, ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// 32-bit-offset buffer loads (wave-uniform descriptor, per-lane voffset constant over the launch, the tile's row offset in the
// scalar operand): no 64-bit address arithmetic and no row clamping in the loop — a row past `num_records` reads as 0 without
// touching memory.  aux = 2: non-temporal (every plane byte is used once per launch).
template <int W> __device__ inline void bload(__amdgpu_buffer_rsrc_t r, int voff, int soff, uint32_t (&w)[W]) {
  if constexpr (W == 4) {
    const auto x = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 2);
    w[0] = x[0]; w[1] = x[1]; w[2] = x[2]; w[3] = x[3];
  } else if constexpr (W == 3) {
    const auto x = __builtin_amdgcn_raw_buffer_load_b96(r, voff, soff, 2);
    w[0] = x[0]; w[1] = x[1]; w[2] = x[2];
  } else if constexpr (W == 2) {
    const auto x = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 2);
    w[0] = x[0]; w[1] = x[1];
  } else {
    w[0] = __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 2);
  }
}
__device__ inline float bload_f32(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
template <int W> __device__ inline void bstore(__amdgpu_buffer_rsrc_t r, int voff, int soff, const uint32_t (&w)[W]) {
  if constexpr (W == 4) {
    const u32x4 x = {w[0], w[1], w[2], w[3]};
    __builtin_amdgcn_raw_buffer_store_b128(x, r, voff, soff, 0);
  } else if constexpr (W == 2) {
    const u32x2 x = {w[0], w[1]};
    __builtin_amdgcn_raw_buffer_store_b64(x, r, voff, soff, 0);
  } else {
    __builtin_amdgcn_raw_buffer_store_b32(w[0], r, voff, soff, 0);
  }
}
__device__ inline __amdgpu_buffer_rsrc_t make_rsrc(const void* base, int64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)(bytes < 0x7FFFFFFF ? (bytes > 0 ? bytes : 0) : 0x7FFFFFFF),
                                           0x00020000);
}
// field t (compile-time after unrolling) of a piece of 16 BITS-bit fields held in BITS/2 dwords, as fp32
template <int BITS, int W> __device__ inline float field_f32(const uint32_t (&w)[W], int t) {
  const int bit = BITS * t, wi = bit / 32, off = bit % 32;
  const uint32_t mask = (1u << BITS) - 1u;
  uint32_t f;
  if (off + BITS <= 32) f = (w[wi] >> off) & mask;
  else f = __builtin_amdgcn_alignbit(w[wi + 1 < W ? wi + 1 : wi], w[wi], off) & mask;
  return (float)f;
}
// 6-bit fields without a conversion (round 5): the 32-bit window that starts at bit `s` of the piece (one shift / v_alignbit) puts
// a field into mantissa bits [P, P + 6) of an fp32 whose exponent makes the mantissa's bit P worth 1 — `(win & mask) | magic`
// (one v_and_or_b32) IS the float 2^(23-P) + field, exactly; the constant leaves through the weight sum like the offset-binary
// bias.  P = 17 (64 + f) and P = 11 (4096 + f) hold two NEIGHBOURING fields of one window: 1.5 instructions per field (values:
// the 4096 costs 6 bits of the accumulator — 2^-12 of a field step per addition, the output tolerance is 2^-7 of full scale);
// P = 17 only: 2 per field (keys: the fp32 logits keep their precision).  r04: shift + and + v_cvt_f32_u32, 3 for a field that
// straddles two dwords = 2.5 per field.
constexpr float kMagic6Hi = 64.0f, kMagic6Lo = 4096.0f;
template <int W> __device__ inline uint32_t piece_window(const uint32_t (&w)[W], int s) {   // bits [s, s + 32) of the piece (s compile-time)
  if (s < 0) return w[0] << (-s);
  const int wi = s / 32, sh = s % 32;
  if (sh == 0) return w[wi];
  if (wi + 1 < W) return __builtin_amdgcn_alignbit(w[wi + 1], w[wi], sh);
  return w[wi] >> sh;
}
__device__ inline float magic6_hi(uint32_t win) { return __uint_as_float(and_or_b32(win, 0x007E0000u, 0x42800000u)); }   // 64 + field at [17, 23)
__device__ inline float magic6_lo(uint32_t win) { return __uint_as_float(and_or_b32(win, 0x0001F800u, 0x45800000u)); }   // 4096 + field at [11, 17)

// MAGIC (keys): 16-bit outputs only, as fma_piece's — the 64 + f fields and the 96 qsum taken out cost an fp32 logit ~3 bits
template <int BITS, int W, bool MAGIC = (BITS == 6)>
__device__ inline float dot_piece(const uint32_t (&w)[W], const float (&qv)[16]) {
  float a0 = 0.f, a1 = 0.f;
  if constexpr (MAGIC) {       // every field at [17, 23): sum_t q_t (64 + f_t); the caller takes 64 qsum out
#pragma unroll
    for (int t = 0; t < 16; t += 2) {
      a0 = fmaf(qv[t], magic6_hi(piece_window<W>(w, 6 * t - 17)), a0);
      a1 = fmaf(qv[t + 1], magic6_hi(piece_window<W>(w, 6 * (t + 1) - 17)), a1);
    }
    return a0 + a1;
  }
#pragma unroll
  for (int t = 0; t < 16; t += 2) {
    a0 = fmaf(qv[t], field_f32<BITS, W>(w, t), a0);
    a1 = fmaf(qv[t + 1], field_f32<BITS, W>(w, t + 1), a1);
  }
  return a0 + a1;
}
// (magic form: o[t] gains wgt * (4096 + f) for even t, wgt * (64 + f) for odd t: piece_bias6(t) * the weight sum is taken out at the end)
__device__ inline float piece_bias6(int t) { return (t & 1) ? kMagic6Hi : kMagic6Lo; }
// MAGIC: the magic form for 16-bit outputs only.  An fp32 output keeps the bits the 4096 would cost: through it the (6, 6) output
// sat ~2^-17 of full scale off exact math, 12x the oracle's error (tests/test_gpu_pq_regimes.py); extract + convert keeps it at
// the (8, 8) path's
template <int BITS, int W, bool MAGIC = (BITS == 6)>
__device__ inline void fma_piece(float (&o)[16], const uint32_t (&w)[W], float wgt) {
  if constexpr (MAGIC) {
#pragma unroll
    for (int t = 0; t < 16; t += 2) {
      const uint32_t win = piece_window<W>(w, 6 * t - 11);     // field t at [11, 17), field t + 1 at [17, 23)
      o[t] = fmaf(wgt, magic6_lo(win), o[t]);
      o[t + 1] = fmaf(wgt, magic6_hi(win), o[t + 1]);
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < 16; ++t) o[t] = fmaf(wgt, field_f32<BITS, W>(w, t), o[t]);
}

// ---- the quantised-query form (include/spatten.h "Quantised query"): integer group sum and the piece's integer dot ----------
template <int CTRL> __device__ inline int dpp_mov_i(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, true); }
template <int WIDTH> __device__ inline int group_sum_i(int v) {
  static_assert(WIDTH == 4 || WIDTH == 8, "group width");
  v += dpp_mov_i<kDppXor1>(v);
  v += dpp_mov_i<kDppXor2>(v);
  if (WIDTH == 8) v += dpp_mov_i<kDppHalfMirror>(v);
  return v;
}
// The lane's 16 quantised query elements packed against the piece's dwords.  8-bit fields (byte t of the piece = field t): qp[j] =
// elements 4j .. 4j + 3.  Nibble fields (nibble t at bit 4t; w & 0x0F0F0F0F = the even fields of a dword as bytes, (w >> 4) &
// 0x0F0F0F0F the odd ones): qp[2j] = the even, qp[2j + 1] = the odd elements of dword j.
template <int KBITS> __device__ inline void qint_pack(const int (&qi)[16], uint32_t (&qp)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (KBITS == 8) qp[j] = pack_i8x4(qi[4 * j], qi[4 * j + 1], qi[4 * j + 2], qi[4 * j + 3]);
    else qp[j] = pack_i8x4(qi[8 * (j / 2) + (j & 1)], qi[8 * (j / 2) + (j & 1) + 2], qi[8 * (j / 2) + (j & 1) + 4], qi[8 * (j / 2) + (j & 1) + 6]);
  }
}
// sum_t q_t field_t over the lane's piece + `init` (v_dot4c_i32_i8, exact).  8-bit fields hold msb + 128: the XOR of the sign bits
// turns a byte into msb itself (two's complement).  Nibble fields are in [0, 15], positive as signed bytes: the MSB plane's + 8
// leaves through init = -8 sum_t q_t, the LSB plane has none.
template <int KBITS, int W> __device__ inline int qint_dot(const uint32_t (&w)[W], const uint32_t (&qp)[4], int init) {
  int a = init;
  if constexpr (KBITS == 8) {
#pragma unroll
    for (int j = 0; j < 4; ++j) a = __builtin_amdgcn_sdot4((int)qp[j], (int)(w[j] ^ 0x80808080u), a, false);
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      a = __builtin_amdgcn_sdot4((int)qp[2 * j], (int)(w[j] & 0x0F0F0F0Fu), a, false);
      a = __builtin_amdgcn_sdot4((int)qp[2 * j + 1], (int)((w[j] >> 4) & 0x0F0F0F0Fu), a, false);
    }
  }
  return a;
}

// APP (round 5): the MSB pass that also appends the step's row — its own instantiation: carried as a run-time branch the path cost every
// OTHER caller 0.8-1.0 us per pass (a branch around the new token's loads behind the first tile breaks the exact vmcnt the
// pipelined tiles rely on: same-call A/B, (4,8) 15.5 vs 14.65 us).
// SO (scores only): no V traffic and no output — the stash, the fp32 logits (msb_logit: pass 1 all heads, the refetch pass
// rewrites the flagged heads' rows with their final logits), lse and need_lsb; the kept-row select and the gather follow
// QI: the quantised-query form — only the prologue (quantise, pack, export) and the per-row logit differ
// CF (cascade fold, spatten_attn_decode_pq_cascade): the FULL step with SO's fold — its own instantiation, as APP is and for APP's
// reason: every other instantiation keeps its code.  The MSB pass adds the previous step's probability of row j to acc[h, j] before it
// overwrites msb_logit[b, h, j] (the row's c == 0 thread, rows j < prev_len of its split: ONE add per (b, h, j) and step); the refetch
// pass leaves the flagged heads' final logits in msb_logit, so after the step msb_logit holds the logits the output came from.
// prev_lse is ONE buffer, read and written in the same step:
//   MSB pass: every wave of every split loads prev_lse[unit] before its first tile and consumes it no later than its last tile (the
//   fold is the only reader).  A workgroup publishes its partial only behind the __syncthreads() that follows every wave's last
//   tile, and the merging workgroup — the last split (polling form) or the last arriver (ticket form) — stores prev_lse[unit] only
//   after it has SEEN every split's partial carry this launch's tag.  A store issued after the loads' values were consumed cannot
//   reach them: the merger's store is ordered behind every read of the unit.  One split: the same __syncthreads().
//   Refetch pass (the compact grid included): it never READS prev_lse — it folds nothing — and it starts after the MSB pass has
//   ended (stream order), so its merger's store needs no argument inside the launch; which split merges does not matter.
// The MSB pass publishes for every head (the MSB-only statistics, final for a confident head), the refetch pass overwrites the
// flagged ones: exactly the two stores `lse` sees.
// RG (ragged batch, spatten_pq_decode_args_t::step_state_sb != 0): one step state per sequence — its own instantiation of the DYN
// forms, as APP is: every other instantiation keeps its code.  Everything the kernel takes from the state — word 0 (the length),
// word 3 (the cascade fold's rows; the scores-only fold has no RG form) and the two staged rotary rows behind the header that the host bakes into p.cos /
// p.sin (row 0: the query's, row 1: the appended key's) — moves by b * step_sb bytes: b = blockIdx.z is uniform over the workgroup,
// so this is scalar address arithmetic in front of the first request.  The length then differs per sequence and with it `owns_new`,
// `hi`, the stash descriptors and the append's N <= p.N guard; the grid, the workspace and the merges are laid out for the bound.
// CF && RG (spatten_attn_decode_pq_cascade_ragged): sequence b folds the rows of ITS previous step (its word 3) into acc + b *
// acc_sb — still one add per (b, h, j) and step, now into an element no other workgroup adds to (the shared-state form's batch
// rows meet in one [H, L] accumulator; here they do not), so the result has one value at every batch size.  The ordering argument
// for prev_lse above is per UNIT and mentions no length: a unit's splits are the same S workgroups whatever its sequence's length
// is (the grid is laid out for the bound; a split whose chunk lies past length_b scores no row, folds no row — j < hi fails — and
// still publishes its empty partial behind the same __syncthreads()), each of them loads prev_lse[unit] before its first tile,
// and the unit's merger stores it only after all S partials carry the tag.  Another sequence's length moves only that sequence's
// units, whose prev_lse entries are other addresses.
template <typename T, int D, int KB, int VB, int PASS, bool DYN, int UP, bool APP = false, bool SO = false, bool QI = false,
          bool CF = false, bool RG = false>
__global__ __launch_bounds__(kPqvThreads) void pqv_decode_kernel(const PqvParams<T> p_in) {
  static_assert(!RG || (DYN && !SO), "one state per sequence: the device-length forms of the full step (CF: the cascade fold)");
  static_assert(!QI || (sizeof(T) < 4 && KB != 6 && !APP && !SO), "the quantised-query form: 16-bit dtypes, (8, 8) / (4, 8), no append, full P.V");
  static_assert(!CF || (!APP && !SO && !QI), "the cascade form: the full step, no in-launch append, fp32 query");
  PqvParams<T> p = p_in;                         // (the compact refetch pass picks its split layout by the number of flagged heads)
  constexpr int LPR = D / 16;                    // lanes per row: lane c owns the row's piece c (16 elements)
  constexpr int RPI = kPqvThreads / LPR;         // rows per row-group
  constexpr int TILE = RPI * UP;
  constexpr int HALF = D / 2;
  constexpr int G = (kPqvThreads / D) > 0 ? (kPqvThreads / D) : 1;
  constexpr int KBITS = (PASS == 1) ? KB : 4;    // pass 2 reads the LSB nibbles
  constexpr int KW = KBITS / 2;                  // dwords of this lane's key piece
  constexpr int KROW = D * KBITS / 8;            // bytes of a key-plane row
  constexpr int VW = VB / 2;
  constexpr int VROW = D * VB / 8;
  constexpr bool VMAGIC = VB == 6 && sizeof(T) < 4;     // (fma_piece)
  constexpr bool KMAGIC = KBITS == 6 && sizeof(T) < 4;  // (dot_piece)
  using V8 = Vec8<T>;

  __shared__ float s_o[kPqvWaves][D + 2];
  __shared__ unsigned s_ticket;

  const int tid = threadIdx.x;
  const int c = tid % LPR;
  const int r = tid / LPR;
  const int wave = tid / kWave;
  const int lane = tid % kWave;

  int split = blockIdx.x;
  const int b = blockIdx.z;
  if constexpr (RG) {
    const int64_t so = (int64_t)b * p.step_sb;
    p.step = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(p.step) + so);
    p.cos = reinterpret_cast<const T*>(reinterpret_cast<const char*>(p.cos) + so);
    p.sin = reinterpret_cast<const T*>(reinterpret_cast<const char*>(p.sin) + so);
  }
  int y = blockIdx.y;
  if (PASS == 2 && p.compact) {
    int f = 0;
    if (lane < p.n_act) f = p.need[b * p.H + (p.head_ids ? p.head_ids[lane] : lane)] != 0;
    unsigned long long m = __ballot(f);
    const int cnt = __popcll(m);
    int rank = blockIdx.y;
    if (2 * cnt > p.n_act) {
      // MANY flagged heads (the every-head-flagged worst case): the fine layout would be 4x the workgroups and 32 partials per
      // merge — the first S1 x cnt workgroups of the grid take pass 1's coarser layout instead, the rest leave
      const int lin = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
      if (lin >= p.S1 * cnt) return;
      rank = lin / p.S1; split = lin - rank * p.S1;
      p.S = p.S1; p.chunk = p.chunk1;
    } else if (rank >= cnt) {
      return;                                        // fewer flagged heads than this row of the grid
    }
    for (int i = 0; i < rank; ++i) m &= m - 1ull;
    y = __builtin_ctzll(m);
  }
  const int h = p.head_ids ? p.head_ids[y] : y;
  const int hkv = (p.Hkv == p.H) ? h : h / (p.H / p.Hkv);
  const int unit = b * p.H + h;
  if (PASS == 2 && p.need[unit] == 0) return;    // confident head: pass 1 already produced its output

  int n_dyn = 0, pl_dyn = 0;
  if (DYN) n_dyn = p.step[opaque_lane(0)];       // requested FIRST (in-order returns), read after the tile loads went out
  constexpr bool fold = (SO || CF) && PASS == 1;       // (the cascade fold: prev_len = 0 / acc == NULL turn it off at run time)
  float prev_ml[2] = {0.f, 1.f};
  if (fold) {
    if (DYN) pl_dyn = p.step[3 + opaque_lane(0)];
    const float* ml = p.prev_lse + 2 * unit + opaque_lane(0);
    prev_ml[0] = ml[0]; prev_ml[1] = ml[1];
  }
  const int lo = split * p.chunk;
  const int rl = min(lo + p.chunk, p.N);         // static row limit of the loads (DYN: p.N is the bound): rows >= rl read as 0

  const uint8_t* kpb = (PASS == 1) ? p.pl.km + b * p.pl.km_sb + hkv * p.pl.km_sh : p.pl.kl + b * p.pl.kl_sb + hkv * p.pl.kl_sh;
  float* lgb = p.pl.lg + b * p.pl.lg_sb + h * p.pl.lg_sh;
  const __amdgpu_buffer_rsrc_t rs_k = make_rsrc(kpb, (int64_t)rl * KROW);
  const __amdgpu_buffer_rsrc_t rs_ks = make_rsrc(p.pl.ks + b * p.pl.sc_sb + hkv * p.pl.sc_sh, (int64_t)rl * 4);
  const __amdgpu_buffer_rsrc_t rs_v = make_rsrc(p.pl.vq + b * p.pl.vq_sb + hkv * p.pl.vq_sh, (int64_t)rl * VROW);
  const __amdgpu_buffer_rsrc_t rs_vs = make_rsrc(p.pl.vs + b * p.pl.sc_sb + hkv * p.pl.sc_sh, (int64_t)rl * 4);
  // (the fold's old logits: a descriptor of 0 records when nothing is folded — the loads then touch no memory)
  const __amdgpu_buffer_rsrc_t rs_lg = make_rsrc(lgb, (PASS == 2 || (fold && p.acc != nullptr && (!CF || DYN || p.prev_len > 0))) ? (int64_t)rl * 4 : 0);
  // Rows of a tile (round 5): thread-row r owns the UP CONSECUTIVE rows t0 + r UP + u (r04: t0 + u RPI + r) — a wave's rows of a
  // tile are then one contiguous run, the UP row scales of a lane are ONE 16-byte load per plane (r04: a 4-byte load per
  // row-group and plane — half of the kernel's memory instructions carried 32 bytes per wave), and a lane's UP stash entries /
  // MSB logits leave as one store.  The plane rows of one wave instruction are UP rows apart: still whole 64- / 96- / 128-byte rows.
  static_assert(UP == 4 || UP == 2, "row scales travel as one 8- or 16-byte load");
  const int vo_k = r * (UP * KROW) + c * (2 * KBITS), vo_v = r * (UP * VROW) + c * (2 * VB), vo_s = r * (UP * 4);

  struct Tile {
    uint32_t kw[UP][KW]; uint32_t ks[UP];        // this lane's piece of the key row + the rows' scales (fp32 bits)
    uint32_t vw[UP][VW]; uint32_t vs[UP];
    uint32_t lg[UP];                             // PASS 2: the MSB logits pass 1 left; SO pass 1: the previous step's logits
  };
  Tile tile_a, tile_b;
  auto issue = [&](Tile& tl, int t0) {
    bload<UP>(rs_ks, vo_s, t0 * 4, tl.ks);
    if (PASS == 2 || fold) bload<UP>(rs_lg, vo_s, t0 * 4, tl.lg);
#pragma unroll
    for (int u = 0; u < UP; ++u) bload<KW>(rs_k, vo_k, (t0 + u) * KROW, tl.kw[u]);   // (wave-uniform part in the scalar offset)
    if (!SO) {
      bload<UP>(rs_vs, vo_s, t0 * 4, tl.vs);
#pragma unroll
      for (int u = 0; u < UP; ++u) bload<VW>(rs_v, vo_v, (t0 + u) * VROW, tl.vw[u]);
    }
  };

  typename V8::raw q_raw[4];
  {
    const T* qp = p.q + b * p.q_sb + h * p.q_sh;
    const int pq = min(max(p.pos_q, 0), p.table_rows - 1);
    q_raw[0] = V8::ldg(qp + 8 * c);
    q_raw[1] = V8::ldg(qp + HALF + 8 * c);
    q_raw[2] = V8::ldg(p.cos + (int64_t)pq * HALF + 8 * c);
    q_raw[3] = V8::ldg(p.sin + (int64_t)pq * HALF + 8 * c);
  }
  issue(tile_a, lo);
  // APPEND (round 5, MSB pass): every split's first thread-row requests the new token's K / V pieces and the rotary row of its slot
  // behind the first tile (static addresses); the split that owns row N - 1 rotates, stores the cache rows, packs and stores the row
  // of every plane and scores it FROM ITS REGISTERS as one extra key (the tiles never read it; the refetch pass is another launch)
  constexpr bool app = APP && PASS == 1;
  typename V8::raw nk_raw[2], nv_raw[2], nr_raw[2];
  if constexpr (app) {             // (EVERY thread, unconditionally: no control flow between the tile's loads and their first wait)
    const T* kp = p.k_new + b * p.new_sb + hkv * p.new_sh;
    const T* vp = p.v_new + b * p.new_sb + hkv * p.new_sh;
    nk_raw[0] = V8::ldg(kp + 8 * c); nk_raw[1] = V8::ldg(kp + HALF + 8 * c);
    nv_raw[0] = V8::ldg(vp + 8 * c); nv_raw[1] = V8::ldg(vp + HALF + 8 * c);
    nr_raw[0] = V8::ldg(p.cos + (int64_t)p.nr_row * HALF + 8 * c);
    nr_raw[1] = V8::ldg(p.sin + (int64_t)p.nr_row * HALF + 8 * c);
  }
  const unsigned gen = p.ws_cnt[(p.S > 1 ? 2 * unit + 1 : 0) + opaque_lane(0)];
  __builtin_amdgcn_sched_barrier(0);

  const int N = DYN ? __builtin_amdgcn_readfirstlane(n_dyn) : p.N;
  const int hi_all = min(lo + p.chunk, N);
  // (DYN: p.N is the launch's BOUND = the planes' capacity — a replay past it must not write beyond the planes: ADVICE r05)
  const bool owns_new = app && lo <= N - 1 && N - 1 < hi_all && (!DYN || N <= p.N);      // (wave-uniform)
  const int hi = owns_new ? hi_all - 1 : hi_all;                   // rows the tiles score

  // ---- the rotated query: fp32 values (they ARE model-dtype values: rope_pair rounds) in piece order; for the nibble planes
  // also packed for the pair-dot trick (common.h NibbleDot: nibble k of a dword pairs with nibble k + 4)
  float qv[16];
  float qsum = 0.f;
  typename NibbleDot<T>::packed qn[2];
  {
    float xlo[8], xhi[8], cc[8], ss[8], ylo[8], yhi[8];
    V8::unpack(q_raw[0], xlo);
    V8::unpack(q_raw[1], xhi);
    V8::unpack(q_raw[2], cc);
    V8::unpack(q_raw[3], ss);
    rope_pair<T>(xlo, xhi, cc, ss, ylo, yhi);
#pragma unroll
    for (int i = 0; i < 8; ++i) { qv[i] = ylo[i]; qv[8 + i] = yhi[i]; qsum += ylo[i] + yhi[i]; }
    if (KBITS == 4) {
      float e0[8], e1[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) { e0[i] = ylo[i]; e1[i] = yhi[i]; }
      qn[0] = NibbleDot<T>::prep(e0);
      qn[1] = NibbleDot<T>::prep(e1);
    }
  }
  const float rsqrt_d = 1.0f / p.sqrt_d;
  // ---- QI: amax over the head (every row-group holds the same query: the group max IS the head's), q_scale = amax / qmax,
  // q_int = the nearest rounding of qr / q_scale (pq_qint.h: the routine the grouped MSB pass shares), packed against the piece's
  // dwords; split 0's first row-group exports both — buffer
  // stores whose descriptor is empty for every other workgroup and whose offset is out of range for every other lane: no branch
  uint32_t qp[4] = {0u, 0u, 0u, 0u};
  int qbias = 0;
  float cq = 0.f;
  if constexpr (QI) {
    float amax = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) amax = fmaxf(amax, fabsf(qv[t]));
    amax = fmaxf(amax, dpp_mov<kDppXor1>(amax));
    amax = fmaxf(amax, dpp_mov<kDppXor2>(amax));
    if (LPR == 8) amax = fmaxf(amax, dpp_mov<kDppHalfMirror>(amax));
    const float qmaxf = (float)p.qmax;
    float qs, qs_div;
    qint_scale(amax, qmaxf, qs, qs_div);
    int qi[16];
    int qsum_i = 0;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      qi[t] = qint_round(qv[t], qs_div, qmaxf);
      qsum_i += qi[t];
    }
    qint_pack<KBITS>(qi, qp);
    qbias = (PASS == 1 && KBITS == 4) ? -8 * qsum_i : 0;
    cq = qs * (16.f * rsqrt_d);
    if constexpr (PASS == 1) {
      const bool exporter = blockIdx.x == 0;                            // (wave-uniform; pass 1 is never compacted)
      const __amdgpu_buffer_rsrc_t rs_qi = make_rsrc(p.qi_out + b * p.qi_sb + h * p.qi_sh, exporter ? D : 0);
      const __amdgpu_buffer_rsrc_t rs_qs = make_rsrc(p.qs_out + unit, exporter ? 4 : 0);
      const uint32_t wlo[2] = {pack_i8x4(qi[0], qi[1], qi[2], qi[3]), pack_i8x4(qi[4], qi[5], qi[6], qi[7])};
      const uint32_t whi[2] = {pack_i8x4(qi[8], qi[9], qi[10], qi[11]), pack_i8x4(qi[12], qi[13], qi[14], qi[15])};
      const int vo_q = (r == 0) ? 8 * c : 0x40000000;
      bstore<2>(rs_qi, vo_q, 0, wlo);                                   // elements 8c .. 8c + 7
      bstore<2>(rs_qi, vo_q, HALF, whi);                                // elements d/2 + 8c ..
      const uint32_t wq[1] = {__float_as_uint(qs)};
      bstore<1>(rs_qs, tid == 0 ? 0 : 0x40000000, 0, wq);
    }
  }
  // stash / MSB-logit stores without branches: buffer stores whose descriptor ends at row `hi` (a row past it is dropped by
  // the bounds check) and whose per-lane offset is out of range for every lane but the row's first (c != 0)
  T* stashp = p.scores ? p.scores + b * p.sc_sb + h * p.sc_sh : nullptr;
  const __amdgpu_buffer_rsrc_t rs_st = make_rsrc(stashp, stashp ? (int64_t)hi * (int64_t)sizeof(T) : 0);
  const __amdgpu_buffer_rsrc_t rs_lgw = make_rsrc(lgb, (PASS == 1 || SO || CF) ? (int64_t)hi * 4 : 0);
  const int prev_len = !fold ? 0 : (p.acc == nullptr) ? 0 : DYN ? __builtin_amdgcn_readfirstlane(pl_dyn) : p.prev_len;
  float* accp = (fold && p.acc != nullptr) ? p.acc + h * p.acc_sh : nullptr;
  if constexpr (CF && RG) { if (accp) accp += (int64_t)b * p.acc_sb; }
  // (exp / sum with a true division: the same bits as spatten_importance_accumulate's fold of the same row, so a step folded
  //  here and a step folded by the flush add identical values — an eager loop and a graph that binds mid-turn agree)
  const float casc_m = (prev_ml[0] == -INFINITY) ? 0.f : prev_ml[0], casc_l = prev_ml[1];
  const int vo_st = (c == 0) ? r * (UP * (int)sizeof(T)) : 0x40000000, vo_lw = (c == 0) ? r * (UP * 4) : 0x40000000;

  float m_run = -INFINITY, l_run = 0.f, off_run = 0.f;
  float o16[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) o16[i] = 0.f;

  if constexpr (app) {
    if (owns_new && tid < LPR) {
      float xlo[8], xhi[8], cc[8], ss[8], ylo[8], yhi[8], va[8], vb[8];
      V8::unpack(nk_raw[0], xlo);
      V8::unpack(nk_raw[1], xhi);
      V8::unpack(nr_raw[0], cc);
      V8::unpack(nr_raw[1], ss);
      rope_pair<T>(xlo, xhi, cc, ss, ylo, yhi);
      const int64_t dst = b * p.kv_sb + hkv * p.kv_sh + (int64_t)(N - 1) * D;
      if (p.kc) { V8::stg(p.kc + dst + 8 * c, nk_raw[0]); V8::stg(p.kc + dst + HALF + 8 * c, nk_raw[1]); }
      V8::stg(p.krc + dst + 8 * c, V8::pack(ylo));
      V8::stg(p.krc + dst + HALF + 8 * c, V8::pack(yhi));
      V8::stg(p.vc + dst + 8 * c, nv_raw[0]);
      V8::stg(p.vc + dst + HALF + 8 * c, nv_raw[1]);
      V8::unpack(nv_raw[0], va);
      V8::unpack(nv_raw[1], vb);
      float kx[16], vx[16];
#pragma unroll
      for (int e = 0; e < 8; ++e) { kx[e] = ylo[e]; kx[8 + e] = yhi[e]; vx[e] = va[e]; vx[8 + e] = vb[e]; }
      PlanePieces<D, KB, VB> pp;
      pack_plane_pieces<D, KB, VB>(kx, vx, pp);
      store_plane_words<D, KB, VB>(p.pl, b, hkv, N - 1, c, pp);
      // its MSB logit, exactly as a tile row's
      float a;
      if (KBITS == 4) a = NibbleDot<T>::dot(qn[0], pp.wm[0], 8.f) + NibbleDot<T>::dot(qn[1], pp.wm[KW - 1], 8.f);
      else a = fmaf(-((float)(1 << (KB - 1)) + (KMAGIC ? kMagic6Hi : 0.f)), qsum, dot_piece<KBITS, KW, KMAGIC>(pp.wm, qv));
      a = group_sum<LPR>(a);
      const float sn = a * (pp.ks * (16.f * rsqrt_d));
      if (c == 0) {
        if (stashp) stashp[N - 1] = DT<T>::from_f32(sn);
        lgb[N - 1] = sn;
      }
      m_run = sn; l_run = 1.f;                           // the first key of this thread-row's softmax
      if (!SO) {
        const float wgt = pp.vs;
        fma_piece<VB, VW, VMAGIC>(o16, pp.wv, wgt);
        off_run = wgt;
      }
    }
  }
  // every row-group of a tile is computed unconditionally (rows past the split read as zeros); `valid` gates the results
  auto process_tile = [&](Tile& tl, int t0) {
    float sc[UP];
#pragma unroll
    for (int u = 0; u < UP; ++u) {
      float a;
      if constexpr (QI) {    // A = sum_i q_int_i field_i as int32 (|A| < 2^24: the conversion is exact); s = float(A) (key_scale cq)
        const int ai = group_sum_i<LPR>(qint_dot<KBITS, KW>(tl.kw[u], qp, qbias));
        const float s = (float)ai * (__uint_as_float(tl.ks[u]) * (PASS == 1 ? cq : cq * 0.0625f));
        sc[u] = (PASS == 2) ? __uint_as_float(tl.lg[u]) + s : s;
        continue;
      }
      if (KBITS == 4) {      // fields hold msb + 8 (pass 1) / the LSB nibble (pass 2)
        a = NibbleDot<T>::dot(qn[0], tl.kw[u][0], PASS == 1 ? 8.f : 0.f) + NibbleDot<T>::dot(qn[1], tl.kw[u][KW - 1], PASS == 1 ? 8.f : 0.f);
      } else {               // fields hold msb + 2^(KB-1)
        // (an explicit fma: the appended row's logit is computed by the same expression elsewhere and must round the same way)
        a = fmaf(-((float)(1 << (KB - 1)) + (KMAGIC ? kMagic6Hi : 0.f)), qsum, dot_piece<KBITS, KW, KMAGIC>(tl.kw[u], qv));
      }
      a = group_sum<LPR>(a);
      const float s = a * (__uint_as_float(tl.ks[u]) * (PASS == 1 ? 16.f * rsqrt_d : rsqrt_d));
      sc[u] = (PASS == 2) ? s + __uint_as_float(tl.lg[u]) : s;
    }
    if (fold && c == 0) {        // the previous step's probability of key j, before this pass overwrites its logit
#pragma unroll
      for (int u = 0; u < UP; ++u) {
        const int j = t0 + r * UP + u;
        if (j < prev_len && j < hi) atomicAdd(accp + j, __expf(__uint_as_float(tl.lg[u]) - casc_m) / casc_l);
      }
    }
    // stash (:116-119) and the MSB logits: a lane's UP rows are consecutive — one store each when the whole tile lies inside the
    // split (wave-uniform test), else row by row against the descriptor's end
    if (t0 + TILE <= hi) {
      uint32_t lw[UP];
#pragma unroll
      for (int u = 0; u < UP; ++u) lw[u] = __float_as_uint(sc[u]);
      if constexpr (sizeof(T) == 4) {
        if (stashp) bstore<UP>(rs_st, vo_st, t0 * 4, lw);
      } else {
        uint32_t sw[UP / 2];
#pragma unroll
        for (int u = 0; u < UP; u += 2) {
          const T a0 = DT<T>::from_f32(sc[u]), a1 = DT<T>::from_f32(sc[u + 1]);
          sw[u / 2] = (uint32_t)*reinterpret_cast<const unsigned short*>(&a0) | ((uint32_t)*reinterpret_cast<const unsigned short*>(&a1) << 16);
        }
        bstore<UP / 2>(rs_st, vo_st, t0 * 2, sw);
      }
      if (PASS == 1 || SO || CF) bstore<UP>(rs_lgw, vo_lw, t0 * 4, lw);
    } else {
#pragma unroll
      for (int u = 0; u < UP; ++u) {
        const float s = sc[u];
        if constexpr (sizeof(T) == 4) {
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(s), rs_st, vo_st, (t0 + u) * 4, 0);
        } else {
          const T sv = DT<T>::from_f32(s);
          __builtin_amdgcn_raw_buffer_store_b16(*reinterpret_cast<const unsigned short*>(&sv), rs_st, vo_st, (t0 + u) * 2, 0);
        }
        if (PASS == 1 || SO || CF) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(s), rs_lgw, vo_lw, (t0 + u) * 4, 0);
      }
    }
    float m_new = m_run;
#pragma unroll
    for (int u = 0; u < UP; ++u) {
      const int j = t0 + r * UP + u;
      const bool valid = j < hi;
      const float s = valid ? sc[u] : -INFINITY;
      sc[u] = s;
      m_new = fmaxf(m_new, s);
    }
    if (m_new > m_run) {
      const float alpha = __expf(m_run - m_new);
      l_run *= alpha;
      off_run *= alpha;
#pragma unroll
      for (int i = 0; i < 16; ++i) o16[i] *= alpha;
      m_run = m_new;
    }
#pragma unroll
    for (int u = 0; u < UP; ++u) {
      const float pj = __expf(sc[u] - m_run);      // exp(-inf) = 0; m_run is finite once a valid row has been seen
      const float pz = (sc[u] == -INFINITY) ? 0.f : pj;
      l_run += pz;
      if (SO) continue;
      const float wgt = pz * __uint_as_float(tl.vs[u]);
      fma_piece<VB, VW, VMAGIC>(o16, tl.vw[u], wgt);
      off_run += wgt;
    }
  };
  for (int t0 = lo; t0 < hi; t0 += 2 * TILE) {
    issue(tile_b, t0 + TILE);
    __builtin_amdgcn_sched_barrier(0);
    process_tile(tile_a, t0);
    issue(tile_a, t0 + 2 * TILE);
    __builtin_amdgcn_sched_barrier(0);
    if (t0 + TILE < hi) process_tile(tile_b, t0 + TILE);
  }
  {   // the fields hold qv + 2^(VB-1): take the constant out through the weight sum
    const float k = (float)(1 << (VB - 1)) * off_run;
#pragma unroll
    for (int i = 0; i < 16; ++i) o16[i] -= VMAGIC ? fmaf(piece_bias6(i), off_run, k) : k;
  }

  // ---- reconcile the row groups (decode_attn.hip): per-wave max and sums in registers, one LDS hop across the waves ----
  {
    const float mw = wave_max(m_run);
    const float alpha = (m_run == -INFINITY) ? 0.f : __expf(m_run - mw);
    l_run *= alpha;
#pragma unroll
    for (int i = 0; i < 16; ++i) o16[i] *= alpha;
    m_run = mw;
  }
  if (LPR == 4) {
    l_run += dpp_mov<kDppRor8>(l_run);
    l_run += dpp_mov<kDppRor4>(l_run);
#pragma unroll
    for (int i = 0; i < 16; ++i) { o16[i] += dpp_mov<kDppRor8>(o16[i]); o16[i] += dpp_mov<kDppRor4>(o16[i]); }
  } else {
    l_run += dpp_mov<kDppRor8>(l_run);
#pragma unroll
    for (int i = 0; i < 16; ++i) o16[i] += dpp_mov<kDppRor8>(o16[i]);
  }
  l_run = xor32_sum(xor16_sum(l_run));
#pragma unroll
  for (int i = 0; i < 16; ++i) o16[i] = xor32_sum(xor16_sum(o16[i]));
  if (lane < LPR) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      s_o[wave][8 * lane + i] = o16[i];
      s_o[wave][HALF + 8 * lane + i] = o16[8 + i];
    }
    if (lane == 0) { s_o[wave][D] = l_run; s_o[wave][D + 1] = m_run; }
  }
  __syncthreads();
  float o_tot = 0.f, l_tot = 0.f;
  {
    static_assert(kPqvWaves == 4, "the fold of the waves' partials is written out for four");
    const float m0 = s_o[0][D + 1], m1 = s_o[1][D + 1], m2 = s_o[2][D + 1], m3 = s_o[3][D + 1];
    const float m_wg = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
    const float mu = (m_wg == -INFINITY) ? 0.f : m_wg;
    const float w0 = __expf(m0 - mu), w1 = __expf(m1 - mu), w2 = __expf(m2 - mu), w3 = __expf(m3 - mu);
    if (tid < D) o_tot = (s_o[0][tid] * w0 + s_o[1][tid] * w1) + (s_o[2][tid] * w2 + s_o[3][tid] * w3);
    l_tot = (s_o[0][D] * w0 + s_o[1][D] * w1) + (s_o[2][D] * w2 + s_o[3][D] * w3);
    m_run = m_wg;
  }
  T* outp = p.out + b * p.out_sb + h * D;
  // head importance: the MSB pass adds only for confident heads, the refetch pass for the heads it recomputes
  auto add_head_abs = [&](float val, bool active, bool commit) {
    float v = wave_sum(active ? fabsf(DT<T>::round(val)) : 0.f);
    __syncthreads();
    if (lane == 0) s_o[0][wave] = v;
    __syncthreads();
    if (tid == 0 && commit) {
      float tot = (s_o[0][0] + s_o[0][1]) + (s_o[0][2] + s_o[0][3]);
      p.head_abs[unit] += tot;
    }
  };
  if (p.S == 1) {
    if (!SO && tid < D) outp[tid] = DT<T>::from_f32(o_tot / l_tot);
    if (p.lse != nullptr && tid == 0) { float* ls = p.lse + (int64_t)unit * 2; ls[0] = m_run; ls[1] = l_tot; }
    if (CF && tid == 0) { float* ps = p.prev_lse + (int64_t)unit * 2; ps[0] = m_run; ps[1] = l_tot; }   // (behind the __syncthreads above)
    const bool need1 = PASS == 1 && (1.0f / l_tot) < p.thr;                              // max prob = exp(0) / sum
    if (PASS == 1 && tid == 0) p.need[unit] = need1 ? 1 : 0;
    if (!SO && p.head_abs != nullptr) add_head_abs(o_tot / l_tot, tid < D, !need1);
    return;
  }

  // ---- publish the partial; merge (decode_attn.hip's protocol on the same workspace) -------------------------------------
  unsigned long long* ws = p.ws_part + (int64_t)unit * p.ws_unit;
  unsigned long long* part = ws + (int64_t)split * (D + 2);
  const unsigned tag = (gen & 0x7FFFFFFFu) + 1u;
  if (!p.poll_merge) {
    if (tid == kPqvThreads - 1)
      s_ticket = __hip_atomic_fetch_add(p.ws_cnt + 2 * unit, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!SO && tid < D && tid < kPqvThreads - kWave) pqv_store_granule(part + tid, o_tot, tag);     // (SO: (max, sum) only)
  if (tid == D) { pqv_store_granule(part + D, m_run, tag); pqv_store_granule(part + D + 1, l_tot, tag); }
  if (p.poll_merge) {
    if (split != p.S - 1) return;
  } else {
    __syncthreads();
    if (s_ticket != (unsigned)(p.S - 1)) return;
  }
  constexpr int KBm = 8;
  const int Gr = p.S > KBm ? G : 1;
  const int e = tid % D, g = tid / D;
  float mg = -INFINITY, lg = 0.f, og = 0.f;
  bool expired = false;
  if (g < Gr) {
    for (int s0 = g; s0 < p.S; s0 += KBm * Gr) {
      unsigned long long ga[KBm], gm[KBm], gl[KBm];
      int spins = 0;
      bool landed;
      do {
#pragma unroll
        for (int k = 0; k < KBm; ++k) {
          const int sc_ = (s0 + k * Gr) < p.S ? (s0 + k * Gr) : g;
          const unsigned long long* qg = ws + (int64_t)sc_ * (D + 2);
          ga[k] = SO ? ((unsigned long long)tag << 32) : __hip_atomic_load(qg + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          gm[k] = __hip_atomic_load(qg + D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          gl[k] = __hip_atomic_load(qg + D + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        unsigned diff = 0u;
#pragma unroll
        for (int k = 0; k < KBm; ++k)
          diff |= ((unsigned)(ga[k] >> 32) ^ tag) | ((unsigned)(gm[k] >> 32) ^ tag) | ((unsigned)(gl[k] >> 32) ^ tag);
        landed = diff == 0u;
      } while (!landed && ++spins < (1 << 16));
      expired |= !landed;
      float a[KBm], ms[KBm], ls[KBm];
#pragma unroll
      for (int k = 0; k < KBm; ++k) {
        const bool live = (s0 + k * Gr) < p.S;
        a[k] = live ? __uint_as_float((unsigned)ga[k]) : 0.f;
        ms[k] = live ? __uint_as_float((unsigned)gm[k]) : -INFINITY;
        ls[k] = live ? __uint_as_float((unsigned)gl[k]) : 0.f;
      }
      float mn = mg;
#pragma unroll
      for (int k = 0; k < KBm; ++k) mn = fmaxf(mn, ms[k]);
      const float mu = (mn == -INFINITY) ? 0.f : mn;
      const float w0 = __expf(mg - mu);
      og *= w0; lg *= w0;
#pragma unroll
      for (int k = 0; k < KBm; ++k) {
        const float w = __expf(ms[k] - mu);
        og = fmaf(a[k], w, og);
        lg = fmaf(ls[k], w, lg);
      }
      mg = mn;
    }
  }
  if (expired) {
    atomicOr(p.ws_err, 1u);
    og = __builtin_nanf("");
  }
  if (Gr > 1) {
    if (g < Gr) { s_o[g][e] = og; if (e == 0) { s_o[g][D] = mg; s_o[g][D + 1] = lg; } }
    __syncthreads();
    if (g == 0) {
      float mn = mg;
#pragma unroll
      for (int gg = 1; gg < Gr; ++gg) mn = fmaxf(mn, s_o[gg][D]);
      const float mu = (mn == -INFINITY) ? 0.f : mn;
      const float w0 = __expf(mg - mu);
      og *= w0; lg *= w0;
#pragma unroll
      for (int gg = 1; gg < Gr; ++gg) {
        const float w = __expf(s_o[gg][D] - mu);
        og = fmaf(s_o[gg][e], w, og);
        lg = fmaf(s_o[gg][D + 1], w, lg);
      }
      mg = mn;
    }
  }
  if (!SO && g == 0) outp[e] = DT<T>::from_f32(og / lg);
  if (!SO && p.head_abs != nullptr) {
    if (PASS == 1 && tid == 0) s_ticket = (1.0f / lg) < p.thr ? 1u : 0u;
    if (PASS == 1) __syncthreads();
    add_head_abs(og / lg, g == 0, !(PASS == 1 && s_ticket != 0u));
  }
  if (tid == 0) {
    if (p.lse != nullptr) { float* ls = p.lse + (int64_t)unit * 2; ls[0] = mg; ls[1] = lg; }
    if (CF) { float* ps = p.prev_lse + (int64_t)unit * 2; ps[0] = mg; ps[1] = lg; }      // (every split's partial has landed: see the top)
    if (PASS == 1) p.need[unit] = (1.0f / lg) < p.thr ? 1 : 0;
    p.ws_cnt[2 * unit + 1] = gen + 1u;
    if (!p.poll_merge) __hip_atomic_store(p.ws_cnt + 2 * unit, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Workgroups of one instantiation the chip holds at once (for the polling merge: the grid must be co-resident by
// construction).  The runtime's occupancy answer, capped at 2 per CU (every instantiation's LDS / SGPR budget admits two;
// the API can overstate beyond that — MI355X_MICROARCH.md "Residency"), asked once per instantiation.
template <typename K> static int resident_capacity(K kernel) {
  int per_cu = 0, dev = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kPqvThreads, 0) != hipSuccess) per_cu = 1;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
  return std::max(1, std::min(per_cu, 2)) * cus;
}

template <typename T, int D, int KB, int VB, bool SO = false, bool QI = false, bool CF = false>
static int launch_pqv(PqvParams<T>& p, int n_active, bool dyn, bool msb_only, hipStream_t st, bool refetch_only = false,
                      bool cascade_ragged = false) {
  const bool ragged = dyn && p.step_sb != 0;     // (one state per sequence: the RG instantiations)
  // the scores-only fold has no RG instantiation and the cascade fold's is reached from spatten_attn_decode_pq_cascade_ragged alone:
  // spatten_attn_decode_pq_local_v / _pq_cascade refuse a stride before they get here, and a caller that did not must not fall
  // through to the shared-state kernels with a strided state
  if ((SO || CF) && ragged && !(CF && cascade_ragged)) return SPATTEN_ERR_UNSUPPORTED;
  if (cascade_ragged && !(CF && ragged)) return SPATTEN_ERR_INVALID;
  const bool app = p.k_new != nullptr;
  constexpr int UP = kPqvUp;
  const dim3 grid((unsigned)p.S, (unsigned)n_active, (unsigned)p.B), blk(kPqvThreads);
  // (the pass-1 and pass-2 kernels of a profile have different register footprints: the smaller capacity decides)
  // (QI, CF: their own kernels' answer; their register footprint is not the plain kernels')
  static const int cap_static = std::min(resident_capacity(pqv_decode_kernel<T, D, KB, VB, 1, false, UP, false, false, QI, CF>),
                                         resident_capacity(pqv_decode_kernel<T, D, KB, VB, 2, false, UP, false, false, QI, CF>));
  static const int cap_dyn = std::min(resident_capacity(pqv_decode_kernel<T, D, KB, VB, 1, true, UP, false, false, QI, CF>),
                                      resident_capacity(pqv_decode_kernel<T, D, KB, VB, 2, true, UP, false, false, QI, CF>));
  int cap = dyn ? cap_dyn : cap_static;
  if constexpr (!SO && !CF) {
    if (ragged) {            // (asked only when a ragged launch arrives: the shared-state forms keep their answers)
      static const int cap_rg = std::min({resident_capacity(pqv_decode_kernel<T, D, KB, VB, 1, true, UP, false, false, QI, false, true>),
                                          resident_capacity(pqv_decode_kernel<T, D, KB, VB, 2, true, UP, false, false, QI, false, true>),
                                          QI ? 0x7FFFFFFF : resident_capacity(pqv_decode_kernel<T, D, KB, VB, 1, true, UP, !QI, false, QI, false, true>)});
      cap = cap_rg;
    }
  }
  if constexpr (CF) {
    if (ragged) {            // (likewise: asked when the first ragged cascade launch arrives)
      static const int cap_cf_rg = std::min(resident_capacity(pqv_decode_kernel<T, D, KB, VB, 1, true, UP, false, false, false, true, true>),
                                            resident_capacity(pqv_decode_kernel<T, D, KB, VB, 2, true, UP, false, false, false, true, true>));
      cap = cap_cf_rg;
    }
  }
  p.poll_merge = (p.S > 1 && (long long)p.S * n_active * p.B <= cap) ? 1 : 0;
  // ---- the refetch pass (round 6): at the reference traces' rate 2-3 of 30 heads are flagged per layer-step; laid out like pass 1
  // their rows sit on S CUs each and the pass takes as long as if every head were flagged (a CU streams at ~21 B/ns).  So pass 2
  // gets its own, finer split-N (~256-row chunks, <= 64 splits) over a grid whose rows are the RANKS of the flagged heads: a few
  // flagged heads spread over the whole chip, unflagged rows of the grid exit at once.  The merge polls: workgroups are dispatched
  // in order, a head's merging (last) split after its siblings, and no other workgroup ever waits — safe beyond residency.
  PqvParams<T> p2 = p;
  if (!msb_only && n_active <= 64) {
    const int lay = p.S * p.chunk;                       // the layout length pass 1 was laid out for
    const int ws_splits = (int)(p.ws_unit / (D + 2));
    int S2 = std::min({kDecodeMaxSplits, ws_splits, std::max(p.S, ceil_div(lay, 256))});
    const int chunk2 = ceil_div(ceil_div(lay, S2), 8) * 8;
    S2 = ceil_div(lay, chunk2);
    p2.S = S2; p2.chunk = chunk2; p2.compact = 1; p2.n_act = n_active; p2.S1 = p.S; p2.chunk1 = p.chunk;
    p2.poll_merge = S2 > 1 ? 1 : 0;
  }
  const dim3 grid2((unsigned)p2.S, (unsigned)n_active, (unsigned)p.B);
  // (SO: the scores-only kernels need no more registers than the full ones — the capacities above stay a safe bound)
  if constexpr (QI) {      // (no append and no scores-only form: spatten_attn_decode_pq_qint refuses them)
    // (refetch_only: the grouped MSB pass of pq_gqa.hip has run in pass 1's place)
    if (ragged) {
      if (!refetch_only) hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 1, true, UP, false, false, true, false, true>), grid, blk, 0, st, p);
      if (!msb_only) hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 2, true, UP, false, false, true, false, true>), grid2, blk, 0, st, p2);
    } else if (dyn) {
      if (!refetch_only) hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 1, true, UP, false, false, true>), grid, blk, 0, st, p);
      if (!msb_only) hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 2, true, UP, false, false, true>), grid2, blk, 0, st, p2);
    } else {
      if (!refetch_only) hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 1, false, UP, false, false, true>), grid, blk, 0, st, p);
      if (!msb_only) hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 2, false, UP, false, false, true>), grid2, blk, 0, st, p2);
    }
    return hipGetLastError() == hipSuccess ? SPATTEN_OK : SPATTEN_ERR_LAUNCH;
  } else if constexpr (CF) {   // (no append: spatten_attn_decode_pq_cascade[_ragged] refuse it)
    if (ragged) {
      hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 1, true, UP, false, false, false, true, true>), grid, blk, 0, st, p);
      if (!msb_only) hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 2, true, UP, false, false, false, true, true>), grid2, blk, 0, st, p2);
    } else if (dyn) {
      hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 1, true, UP, false, false, false, true>), grid, blk, 0, st, p);
      if (!msb_only) hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 2, true, UP, false, false, false, true>), grid2, blk, 0, st, p2);
    } else {
      hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 1, false, UP, false, false, false, true>), grid, blk, 0, st, p);
      if (!msb_only) hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 2, false, UP, false, false, false, true>), grid2, blk, 0, st, p2);
    }
    return hipGetLastError() == hipSuccess ? SPATTEN_OK : SPATTEN_ERR_LAUNCH;
  } else
  if (ragged) {
    if constexpr (!SO) {
      if (app) hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 1, true, UP, true, false, false, false, true>), grid, blk, 0, st, p);
      else hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 1, true, UP, false, false, false, false, true>), grid, blk, 0, st, p);
      if (!msb_only) hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 2, true, UP, false, false, false, false, true>), grid2, blk, 0, st, p2);
    }                      // (SO: refused at the top)
  } else if (dyn) {
    if (app) hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 1, true, UP, true, SO>), grid, blk, 0, st, p);
    else hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 1, true, UP, false, SO>), grid, blk, 0, st, p);
    if (!msb_only) hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 2, true, UP, false, SO>), grid2, blk, 0, st, p2);
  } else {
    if (app) hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 1, false, UP, true, SO>), grid, blk, 0, st, p);
    else hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 1, false, UP, false, SO>), grid, blk, 0, st, p);
    if (!msb_only) hipLaunchKernelGGL((pqv_decode_kernel<T, D, KB, VB, 2, false, UP, false, SO>), grid2, blk, 0, st, p2);
  }
  return hipGetLastError() == hipSuccess ? SPATTEN_OK : SPATTEN_ERR_LAUNCH;
}

// the local-V extras of spatten_attn_decode_pq_local_v (NULL: the plain profiled step); full: spatten_attn_decode_pq_cascade — the
// fold inside the FULL step (the CF instantiations) instead of the scores-only passes
// acc_sb != 0: spatten_attn_decode_pq_cascade_ragged — one accumulator per sequence (the CF && RG instantiations)
struct PqLvExtra { float* acc; int64_t acc_sh; float* prev_lse; int prev_len; bool full; int64_t acc_sb = 0; };

template <typename T>
static int run_pqv(const spatten_pq_decode_args_t* a, const PlanesDev& pd, hipStream_t st, const PqLvExtra* lv = nullptr,
                   const PqQintExtra* qx = nullptr, bool refetch_only = false) {
  const int kb = a->planes->key_msb_bits;      // (the value width follows: supported profiles are (4, 8), (8, 8), (6, 6))
  const int d = a->head_dim;
  const int n_active = a->head_ids ? a->n_active_heads : a->heads;
  const int units = a->batch * a->heads;
  const int ws_splits = a->workspace_splits > 0 ? a->workspace_splits : kDecodeMaxSplits;
  const int lay = (!a->step_state && a->kv_len_layout > a->kv_len) ? a->kv_len_layout : a->kv_len;
  int S = a->n_splits > 0 ? a->n_splits : decode_auto_splits(a->batch * n_active, d, lay, 2, false);
  if (S > lay) S = lay;
  if (S > kDecodeMaxSplits) S = kDecodeMaxSplits;
  const int chunk = ceil_div(ceil_div(lay, S), 8) * 8;
  S = ceil_div(lay, chunk);
  if (S > 1 && (!a->workspace || S > ws_splits)) return SPATTEN_ERR_INVALID;
  PqvParams<T> p;
  p.q = (const T*)a->q; p.q_sb = a->q_sb; p.q_sh = a->q_sh;
  p.pl = pd;
  p.cos = (const T*)a->cos; p.sin = (const T*)a->sin; p.table_rows = a->table_rows;
  p.step = (const int32_t*)a->step_state;
  p.step_sb = a->step_state ? a->step_state_sb : 0;
  p.pos_q = a->pos_q;
  if (a->step_state) {   // the state's staged rotary rows stand in for the table: row 0 = the query's position
    p.cos = (const T*)((const char*)a->step_state + kStepHeader);
    p.sin = p.cos + 2 * (d / 2); p.table_rows = 2; p.pos_q = 0;
  }
  p.out = (T*)a->out; p.out_sb = a->out_sb;
  p.scores = (T*)a->scores; p.sc_sb = a->sc_sb; p.sc_sh = a->sc_sh;
  p.lse = a->lse; p.head_ids = a->head_ids;
  p.thr = a->threshold; p.need = a->need_lsb; p.head_abs = a->head_abs_acc;
  const size_t cnt_bytes = decode_cnt_bytes((size_t)units);
  p.ws_err = (unsigned*)a->workspace;
  p.ws_cnt = a->workspace ? (unsigned*)((char*)a->workspace + kDecodeWsHeader) : (unsigned*)a->cos;
  p.ws_part = a->workspace ? (unsigned long long*)((char*)a->workspace + kDecodeWsHeader + cnt_bytes) : nullptr;
  p.ws_unit = (int64_t)ws_splits * (d + 2);
  p.B = a->batch; p.H = a->heads; p.Hkv = a->kv_heads; p.N = a->kv_len; p.S = S; p.chunk = chunk;
  p.poll_merge = 0;      // decided per instantiation in launch_pqv (co-residency of the whole grid)
  p.compact = 0; p.n_act = n_active; p.S1 = S; p.chunk1 = chunk;
  p.sqrt_d = sqrtf((float)d);
  p.k_new = (const T*)a->k_new; p.v_new = (const T*)a->v_new; p.new_sb = a->new_sb; p.new_sh = a->new_sh;
  p.kc = (T*)a->k_cache; p.krc = (T*)a->kr_cache; p.vc = (T*)a->v_cache; p.kv_sb = a->kv_sb; p.kv_sh = a->kv_sh;
  p.nr_row = a->step_state ? 1 : std::min(a->kv_len - 1, a->table_rows - 1);
  p.acc = lv ? lv->acc : nullptr; p.acc_sh = lv ? lv->acc_sh : 0; p.acc_sb = lv ? (int)lv->acc_sb : 0;
  p.prev_lse = (lv && lv->acc) ? lv->prev_lse : a->lse; p.prev_len = (lv && lv->acc) ? lv->prev_len : 0;
  p.qi_out = qx ? qx->q_int : nullptr; p.qi_sb = qx ? qx->qi_sb : 0; p.qi_sh = qx ? qx->qi_sh : 0;
  p.qs_out = qx ? qx->q_scale : nullptr; p.qmax = qx ? qx->qmax : 0;
  const bool dyn = a->step_state != nullptr, msb_only = (a->flags & SPATTEN_PQ_MSB_PASS_ONLY) != 0;
#define SPATTEN_PQV(DD, KB, VB)                                                                     \
  do {                                                                                              \
    if constexpr (sizeof(T) < 4 && KB != 6) {                                                       \
      if (qx) return launch_pqv<T, DD, KB, VB, false, true>(p, n_active, dyn, msb_only, st, refetch_only); \
    }                                                                                               \
    if (lv && lv->full) return launch_pqv<T, DD, KB, VB, false, false, true>(p, n_active, dyn, msb_only, st, false, lv->acc_sb != 0); \
    return lv ? launch_pqv<T, DD, KB, VB, true>(p, n_active, dyn, msb_only, st)                     \
              : launch_pqv<T, DD, KB, VB>(p, n_active, dyn, msb_only, st);                          \
  } while (0)
  if (d == 128) {
    if (kb == 4) SPATTEN_PQV(128, 4, 8);
    if (kb == 8) SPATTEN_PQV(128, 8, 8);
    SPATTEN_PQV(128, 6, 6);
  }
  if (kb == 4) SPATTEN_PQV(64, 4, 8);
  if (kb == 8) SPATTEN_PQV(64, 8, 8);
  SPATTEN_PQV(64, 6, 6);
#undef SPATTEN_PQV
}

// ================================================================================================
// Local V pruning over the planes (spatten_attn_decode_pq_local_v): after the scores-only passes, the kept rows of every
// launched head (top-keep of the stash row, ties lowest index first) and P.V over only those rows of the quantised V plane
// with the full-row probabilities of the final fp32 logits (no renormalisation; SpAttenController.scala:546-558,591-612)
// ================================================================================================
constexpr int kLvMaxPer = 1024;         // kept rows per gather workgroup (their (row, weight) pairs live in LDS)
constexpr int kLvMaxSplits = 64;
static inline size_t lv_cnt_bytes(size_t units) { return (units * sizeof(unsigned) + 255) / 256 * 256; }

// kept count of a unit: keep (host form) or ceil(keep_frac * length) in fp64 (device length: what math.ceil gives), in [1, n];
// the device length is clamped to the launch's bound
__device__ inline int pqlv_kept(const int32_t* step, int bound, int keep, double frac, int& n) {
  n = step ? min(step[0], bound) : bound;
  const int k = step ? (int)ceil(frac * (double)n) : keep;
  return max(1, min(k, n));
}

template <typename T>
__global__ __launch_bounds__(kSelThreads) void pqlv_select_kernel(const T* stash, int64_t sc_sb, int64_t sc_sh,
                                                                  const int32_t* head_ids, const int32_t* step, int bound,
                                                                  int keep, double frac, int32_t* idx, int64_t idx_sr, int H) {
  const int h = head_ids ? head_ids[blockIdx.x] : (int)blockIdx.x, b = blockIdx.y;
  int n;
  const int k = pqlv_kept(step, bound, keep, frac, n);
  topk_select_row<T>(stash + b * sc_sb + h * sc_sh, n, k, 0, idx + (int64_t)(b * H + h) * idx_sr);
}

template <typename T>
struct PqlvGatherParams {
  const int32_t* head_ids; const int32_t* step; const int32_t* idx; int64_t idx_sr;
  PlanesDev pl;
  const float* lse; float* prev_lse; float* head_abs;
  T* out; int64_t out_sb;
  float* part; unsigned* cnt;
  int H, Hkv, bound, keep, per; double frac;
};

// grid (S, n_active, B): workgroup `split` takes kept entries [split * per, split * per + per) — (row, weight) pairs into LDS,
// then the rows' V pieces (lane c of a row's D/16 lanes decodes its piece of 16 fields: the plane's piece layout), U rows in
// flight per lane.  Partials go to the workspace; the LAST workgroup of a unit to arrive (ticket, no waiting) adds them in split
// order, writes the output, the head importance, and copies the unit's (max, sum) to prev_lse for the next step's fold.
template <typename T, int D, int VB>
__global__ __launch_bounds__(256) void pqlv_gather_kernel(const PqlvGatherParams<T> p) {
  constexpr int LPR = D / 16, RPI = 256 / LPR, U = 4, VW = VB / 2, VROW = D * VB / 8, HALF = D / 2;
  constexpr float bias = (float)(1 << (VB - 1));
  __shared__ int s_j[kLvMaxPer];
  __shared__ float s_p[kLvMaxPer];
  __shared__ float s_o[4][D];
  __shared__ float s_abs[4];
  __shared__ unsigned s_ticket;
  const int split = blockIdx.x, S = gridDim.x, b = blockIdx.z, tid = threadIdx.x;
  const int c = tid % LPR, r = tid / LPR, lane = tid & 63, wave = tid >> 6;
  const int h = p.head_ids ? p.head_ids[blockIdx.y] : (int)blockIdx.y;
  const int hkv = p.Hkv == p.H ? h : h / (p.H / p.Hkv);
  const int unit = b * p.H + h;
  int n;
  const int k = pqlv_kept(p.step, p.bound, p.keep, p.frac, n);
  const int32_t* ix = p.idx + (int64_t)unit * p.idx_sr;
  const float* lgr = p.pl.lg + b * p.pl.lg_sb + h * p.pl.lg_sh;
  const float* vsr = p.pl.vs + b * p.pl.sc_sb + hkv * p.pl.sc_sh;
  const uint8_t* vqr = p.pl.vq + b * p.pl.vq_sb + hkv * p.pl.vq_sh;
  const float m = p.lse[2 * unit], l = p.lse[2 * unit + 1];
  const float mu = (m == -INFINITY) ? 0.f : m;
  const int i_lo = split * p.per;
  const int cnt_n = max(0, min(p.per, k - i_lo));
  for (int t = tid; t < cnt_n; t += 256) {
    const int j = ix[i_lo + t];
    s_j[t] = j;
    s_p[t] = __expf(lgr[j] - mu) / l * vsr[j];        // probability x the row's value scale
  }
  __syncthreads();
  float o[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) o[e] = 0.f;
  for (int i0 = 0; i0 < cnt_n; i0 += RPI * U) {
    uint32_t w[U][VW];
    float pp[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * RPI + r;
      const bool ok = i < cnt_n;
      const int j = s_j[ok ? i : 0];
      pp[u] = ok ? s_p[i] : 0.f;
      const uint32_t* src = reinterpret_cast<const uint32_t*>(vqr + (int64_t)j * VROW + 2 * VB * c);
#pragma unroll
      for (int x = 0; x < VW; ++x) w[u][x] = src[x];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < 16; ++t) o[t] = fmaf(pp[u], field_f32<VB, VW>(w[u], t) - bias, o[t]);
  }
  // reduce the rows of the wave (lanes with equal c), then the 4 waves
#pragma unroll
  for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] += __shfl_xor(o[e], off, kWave);
  if (lane < LPR)
#pragma unroll
    for (int t = 0; t < 8; ++t) { s_o[wave][8 * lane + t] = o[t]; s_o[wave][HALF + 8 * lane + t] = o[8 + t]; }
  __syncthreads();
  float tot = 0.f;
  if (tid < D) tot = (s_o[0][tid] + s_o[1][tid]) + (s_o[2][tid] + s_o[3][tid]);
  T* orow = p.out + b * p.out_sb + (int64_t)h * D;
  if (S > 1) {
    // partials leave as write-through (agent-scope) stores; the ticket is drawn after they were acknowledged (cascade.hip)
    float* mine = p.part + ((int64_t)unit * kLvMaxSplits + split) * D;
    if (tid < D) __hip_atomic_store(mine + tid, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) s_ticket = __hip_atomic_fetch_add(p.cnt + unit, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_ticket != (unsigned)(S - 1)) return;
    if (tid < D) {
      const float* q = p.part + (int64_t)unit * kLvMaxSplits * D + tid;
      float acc = 0.f;
      for (int s0 = 0; s0 < S; s0 += 8) {          // 8 loads in flight, added in split order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          v[u] = __hip_atomic_load(q + (int64_t)min(s0 + u, S - 1) * D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += (s0 + u < S) ? v[u] : 0.f;
      }
      tot = acc;
    }
    if (tid == 0) __hip_atomic_store(p.cnt + unit, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-arm
  }
  if (tid < D) orow[tid] = DT<T>::from_f32(tot);
  if (p.head_abs != nullptr) {     // head importance (README.md:21) of the value left in `out`, in a fixed order
    const float v = wave_sum(tid < D ? fabsf(DT<T>::round(tot)) : 0.f);
    if (lane == 0) s_abs[wave] = v;
    __syncthreads();
    if (tid == 0) p.head_abs[unit] += (s_abs[0] + s_abs[1]) + (s_abs[2] + s_abs[3]);
  }
  if (p.prev_lse != nullptr && tid < 2) p.prev_lse[2 * unit + tid] = p.lse[2 * unit + tid];
}

template <typename T, int D>
static int launch_pqlv_gather(const PqlvGatherParams<T>& g, int vb, int S, int n_active, int B, hipStream_t st) {
  const dim3 grid((unsigned)S, (unsigned)n_active, (unsigned)B);
  if (vb == 8) hipLaunchKernelGGL((pqlv_gather_kernel<T, D, 8>), grid, dim3(256), 0, st, g);
  else hipLaunchKernelGGL((pqlv_gather_kernel<T, D, 6>), grid, dim3(256), 0, st, g);
  return hipGetLastError() == hipSuccess ? SPATTEN_OK : SPATTEN_ERR_LAUNCH;
}

template <typename T>
static int run_pq_local_v(const spatten_pq_local_v_args_t* la, const PlanesDev& pd, hipStream_t st) {
  const spatten_pq_decode_args_t* a = &la->step;
  const int n_active = a->head_ids ? a->n_active_heads : a->heads;
  const size_t units = (size_t)a->batch * a->heads;
  const bool dyn = a->step_state != nullptr;
  // the gather's slices are sized by a bound of the kept count: ceil(keep_fraction * the layout length) when a fraction is given
  // (the device-length form, and a host-form launch that names its fraction: both then add the same slices in the same order —
  // bit-identical outputs), else the host count itself
  const int lay = (!dyn && a->kv_len_layout > a->kv_len) ? a->kv_len_layout : a->kv_len;
  const int kf = la->keep_fraction > 0.0 ? (int)std::min<double>(std::ceil(la->keep_fraction * (double)lay), (double)lay) : 0;
  const int k_bound = std::max({1, kf, dyn ? 0 : std::min(la->keep, a->kv_len)});
  int per = ceil_div((int)(((long long)k_bound * n_active * a->batch + 1023) / 1024), 16) * 16;
  per = std::max(per, 64);
  per = std::min(per, kLvMaxPer);
  per = std::max(per, ceil_div(k_bound, kLvMaxSplits));
  if (per > kLvMaxPer) return SPATTEN_ERR_UNSUPPORTED;          // more than 65536 kept rows per head
  const int S = ceil_div(k_bound, per);
  unsigned* cnt = (unsigned*)la->workspace;
  float* part = (float*)((char*)la->workspace + lv_cnt_bytes(units));
  int32_t* idx = (int32_t*)((char*)part + units * kLvMaxSplits * (size_t)a->head_dim * sizeof(float));

  PqLvExtra ex{la->importance_acc, la->acc_sh, la->prev_lse, la->prev_len, false};
  int rc = run_pqv<T>(a, pd, st, &ex);                           // MSB pass + refetch pass, scores only
  if (rc != SPATTEN_OK) return rc;
  const int32_t* step = (const int32_t*)a->step_state;
  hipLaunchKernelGGL((pqlv_select_kernel<T>), dim3((unsigned)n_active, (unsigned)a->batch), dim3(kSelThreads), 0, st,
                     (const T*)a->scores, a->sc_sb, a->sc_sh, a->head_ids, step, a->kv_len, la->keep, la->keep_fraction, idx,
                     (int64_t)la->workspace_rows, a->heads);
  if (hipGetLastError() != hipSuccess) return SPATTEN_ERR_LAUNCH;
  PqlvGatherParams<T> g;
  g.head_ids = a->head_ids; g.step = step; g.idx = idx; g.idx_sr = la->workspace_rows;
  g.pl = pd; g.lse = a->lse; g.prev_lse = la->prev_lse; g.head_abs = a->head_abs_acc;
  g.out = (T*)a->out; g.out_sb = a->out_sb; g.part = part; g.cnt = cnt;
  g.H = a->heads; g.Hkv = a->kv_heads; g.bound = a->kv_len; g.keep = la->keep; g.per = per; g.frac = la->keep_fraction;
  if (a->head_dim == 128) return launch_pqlv_gather<T, 128>(g, a->planes->value_bits, S, n_active, a->batch, st);
  return launch_pqlv_gather<T, 64>(g, a->planes->value_bits, S, n_active, a->batch, st);
}

int pq_qint_refetch(const spatten_pq_decode_args_t* a, const PlanesDev& pd, const PqQintExtra& qx, hipStream_t st) {
  if (a->dtype == SPATTEN_BF16) return run_pqv<bf16_t>(a, pd, st, nullptr, &qx, true);
  return run_pqv<f16_t>(a, pd, st, nullptr, &qx, true);
}

int pq_validate(const spatten_pq_decode_args_t* a, PlanesDev& pd) {
  if (!a || a->struct_size != sizeof(spatten_pq_decode_args_t)) return SPATTEN_ERR_INVALID;
  if (!a->q || !a->out || !a->cos || !a->sin || !a->need_lsb || !planes_to_dev(a->planes, pd)) return SPATTEN_ERR_INVALID;
  if (a->batch <= 0 || a->heads <= 0 || a->kv_heads <= 0 || a->heads % a->kv_heads != 0 || a->kv_len <= 0) return SPATTEN_ERR_INVALID;
  if (!a->step_state && (a->pos_q < 0 || a->pos_q >= a->table_rows)) return SPATTEN_ERR_INVALID;
  if (a->kv_len_layout < 0) return SPATTEN_ERR_INVALID;
  if ((a->k_new == nullptr) != (a->v_new == nullptr)) return SPATTEN_ERR_INVALID;
  if (a->k_new && (!a->kr_cache || !a->v_cache)) return SPATTEN_ERR_INVALID;
  const int n_active = a->head_ids ? a->n_active_heads : a->heads;
  if (n_active <= 0 || n_active > a->heads) return SPATTEN_ERR_INVALID;
  if (!ok_dtype(a->dtype)) return SPATTEN_ERR_INVALID;
  if (a->head_dim != 64 && a->head_dim != 128) return SPATTEN_ERR_UNSUPPORTED;
  if (!pq_profile_supported(a->planes->key_msb_bits, a->planes->value_bits)) return SPATTEN_ERR_UNSUPPORTED;
  // one state per sequence (a ragged batch): decode_rows_check's rule — whole 256-byte lines apart, no two states overlapping,
  // checked at every batch size
  if (!step_stride_ok(a->step_state, a->step_state_sb, a->dtype, a->head_dim)) return SPATTEN_ERR_INVALID;
  return SPATTEN_OK;
}

}  // namespace spatten

using namespace spatten;

extern "C" int spatten_attn_decode_pq(const spatten_pq_decode_args_t* a, void* stream) {
  PlanesDev pd;
  const int rc = pq_validate(a, pd);
  if (rc != SPATTEN_OK) return rc;
  if (a->dtype == SPATTEN_BF16) return run_pqv<bf16_t>(a, pd, (hipStream_t)stream);
  if (a->dtype == SPATTEN_F16) return run_pqv<f16_t>(a, pd, (hipStream_t)stream);
  return run_pqv<float>(a, pd, (hipStream_t)stream);
}

extern "C" int spatten_attn_decode_pq_cascade(const spatten_pq_cascade_args_t* ca, void* stream) {
  if (!ca || ca->struct_size != sizeof(spatten_pq_cascade_args_t)) return SPATTEN_ERR_INVALID;
  const spatten_pq_decode_args_t* a = &ca->step;
  PlanesDev pd;
  const int rc = pq_validate(a, pd);
  if (rc != SPATTEN_OK) return rc;
  if (!ca->importance_acc || !ca->prev_lse || !a->lse || !pd.lg) return SPATTEN_ERR_INVALID;
  if (ca->prev_len < 0 || (!a->step_state && ca->prev_len > a->kv_len)) return SPATTEN_ERR_INVALID;
  if (a->step_state_sb != 0) return SPATTEN_ERR_UNSUPPORTED;     // one [H, L] accumulator cannot take sequences of different lengths
  if (a->k_new != nullptr) return SPATTEN_ERR_UNSUPPORTED;       // append with spatten_kv_append_planes first
  PqLvExtra ex{ca->importance_acc, ca->acc_sh, ca->prev_lse, ca->prev_len, true};
  if (a->dtype == SPATTEN_BF16) return run_pqv<bf16_t>(a, pd, (hipStream_t)stream, &ex);
  if (a->dtype == SPATTEN_F16) return run_pqv<f16_t>(a, pd, (hipStream_t)stream, &ex);
  return run_pqv<float>(a, pd, (hipStream_t)stream, &ex);
}

extern "C" int spatten_attn_decode_pq_cascade_ragged(const spatten_pq_cascade_args_t* ca, int64_t acc_batch_stride, void* stream) {
  if (!ca || ca->struct_size != sizeof(spatten_pq_cascade_args_t)) return SPATTEN_ERR_INVALID;
  const spatten_pq_decode_args_t* a = &ca->step;
  PlanesDev pd;
  const int rc = pq_validate(a, pd);                             // (the state stride's rule, at every batch size)
  if (rc != SPATTEN_OK) return rc;
  if (!ca->importance_acc || !ca->prev_lse || !a->lse || !pd.lg) return SPATTEN_ERR_INVALID;
  if (!a->step_state || a->step_state_sb == 0) return SPATTEN_ERR_INVALID;   // the shared state: spatten_attn_decode_pq_cascade
  if (acc_batch_stride < 0) return SPATTEN_ERR_INVALID;
  if (acc_batch_stride == 0) return SPATTEN_ERR_UNSUPPORTED;     // one [H, L] accumulator cannot take sequences of different lengths
  if (acc_batch_stride > 0x7FFFFFFF) return SPATTEN_ERR_UNSUPPORTED;   // (elements; the range of spatten_decode_args_t's acc_sb)
  if (a->k_new != nullptr) return SPATTEN_ERR_UNSUPPORTED;       // append with spatten_kv_append_planes_ragged first
  PqLvExtra ex{ca->importance_acc, ca->acc_sh, ca->prev_lse, 0, true, acc_batch_stride};   // (prev_len: every state's word 3)
  if (a->dtype == SPATTEN_BF16) return run_pqv<bf16_t>(a, pd, (hipStream_t)stream, &ex);
  if (a->dtype == SPATTEN_F16) return run_pqv<f16_t>(a, pd, (hipStream_t)stream, &ex);
  return run_pqv<float>(a, pd, (hipStream_t)stream, &ex);
}

extern "C" int spatten_pq_qint_supported(int dtype, int head_dim, int key_msb_bits, int value_bits, int query_bits) {
  if (dtype != SPATTEN_BF16 && dtype != SPATTEN_F16) return 0;
  if (head_dim != 64 && head_dim != 128) return 0;
  if (!((key_msb_bits == 8 || key_msb_bits == 4) && value_bits == 8)) return 0;
  return query_bits >= 4 && query_bits <= 8;
}

extern "C" int spatten_attn_decode_pq_qint(const spatten_pq_qint_args_t* qa, void* stream) {
  if (!qa || qa->struct_size != sizeof(spatten_pq_qint_args_t)) return SPATTEN_ERR_INVALID;
  if (!qa->q_int || !qa->q_scale || qa->query_bits < 4 || qa->query_bits > 8) return SPATTEN_ERR_INVALID;
  const spatten_pq_decode_args_t* a = &qa->step;
  PlanesDev pd;
  const int rc = pq_validate(a, pd);
  if (rc != SPATTEN_OK) return rc;
  // (the exported query leaves as two 8-byte stores per lane)
  if (((uintptr_t)qa->q_int | (uintptr_t)qa->qi_sb | (uintptr_t)qa->qi_sh) & 7u) return SPATTEN_ERR_INVALID;
  if (a->k_new != nullptr) return SPATTEN_ERR_UNSUPPORTED;
  if (!spatten_pq_qint_supported(a->dtype, a->head_dim, a->planes->key_msb_bits, a->planes->value_bits, qa->query_bits))
    return SPATTEN_ERR_UNSUPPORTED;
  PqQintExtra qx{qa->q_int, qa->qi_sb, qa->qi_sh, qa->q_scale, (1 << (qa->query_bits - 1)) - 1};
  if (a->dtype == SPATTEN_BF16) return run_pqv<bf16_t>(a, pd, (hipStream_t)stream, nullptr, &qx);
  return run_pqv<f16_t>(a, pd, (hipStream_t)stream, nullptr, &qx);
}

extern "C" size_t spatten_pq_local_v_workspace_bytes(int batch, int heads, int head_dim, int max_kv_len) {
  if (batch <= 0 || heads <= 0 || head_dim <= 0 || max_kv_len <= 0) return 0;
  const size_t units = (size_t)batch * heads;
  return lv_cnt_bytes(units) + units * kLvMaxSplits * (size_t)head_dim * sizeof(float) + units * (size_t)max_kv_len * sizeof(int32_t);
}

extern "C" int spatten_attn_decode_pq_local_v(const spatten_pq_local_v_args_t* la, void* stream) {
  if (!la || la->struct_size != sizeof(spatten_pq_local_v_args_t)) return SPATTEN_ERR_INVALID;
  const spatten_pq_decode_args_t* a = &la->step;
  PlanesDev pd;
  const int rc = pq_validate(a, pd);
  if (rc != SPATTEN_OK) return rc;
  if (a->step_state_sb != 0) return SPATTEN_ERR_UNSUPPORTED;     // the select and the gather take ONE kept count from the shared state
  if (a->flags != 0 || !a->scores || !a->lse || !pd.lg || !la->workspace || la->workspace_rows < a->kv_len) return SPATTEN_ERR_INVALID;
  if (a->step_state ? !(la->keep_fraction > 0.0 && la->keep_fraction <= 1.0) : (la->keep <= 0 || !(la->keep_fraction >= 0.0 && la->keep_fraction <= 1.0)))
    return SPATTEN_ERR_INVALID;
  if (la->importance_acc && (!la->prev_lse || la->prev_len < 0 || (!a->step_state && la->prev_len > a->kv_len))) return SPATTEN_ERR_INVALID;
  if (a->dtype == SPATTEN_BF16) return run_pq_local_v<bf16_t>(la, pd, (hipStream_t)stream);
  if (a->dtype == SPATTEN_F16) return run_pq_local_v<f16_t>(la, pd, (hipStream_t)stream);
  return run_pq_local_v<float>(la, pd, (hipStream_t)stream);
}
