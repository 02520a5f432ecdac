// prune_ragged.hip — the prune event of a RAGGED batch (include/spatten.h, "Ragged prune event"): every sequence is pruned by the
// reference's rule at ITS OWN length (kv_cache_token_pruning.py:46,59,80-82), all layers and all sequences in at most three
// launches — select, K/V gather + rotated shadow, accumulator gather.  The lengths are device values (a dense array, or word 0 of
// the per-sequence step states read in place): nothing here reads a host value of a length, allocates or synchronises, so the
// event is captured with the decode steps around it.
//
// What a length decides is data, never geometry: grids, windows' register instantiation and every address bound come from the host
// value `bound`; a sequence's length (clamped to [0, bound]) only selects between the gather, the identity copy and the zero fill.
// The select is prune.hip's (prune_rows.h / select_row.h) on a window whose end differs per workgroup; the row movers are
// kv_compact_kernel's piece-pair mapping with a row map that depends on the sequence.
#include "common.h"
#include "select_row.h"
#include "prune_rows.h"

namespace spatten {

// what every kernel of the event derives from a sequence's length (workgroup-uniform)
struct RaggedRule {
  const int32_t* lens; int lens_step;
  int bound, start, recent, k, num_coming;
  int B, H;                        // H: heads of the cache planes (KV heads)
};
struct RaggedSeq { int len, hi, new_len; bool pruned; };

__device__ __forceinline__ RaggedSeq ragged_seq(const RaggedRule& r, int b) {
  RaggedSeq s;
  s.len = min(max(r.lens[(int64_t)b * r.lens_step], 0), r.bound);
  s.pruned = s.len + r.num_coming > r.start + r.k + r.recent;      // needs_pruning at this sequence's length
  s.hi = s.len - r.recent + r.num_coming;                           // pruned: start + k < hi <= len
  s.new_len = s.pruned ? r.start + r.k + r.recent - r.num_coming : s.len;
  return s;
}
// source row of destination row r < new_len; idx_row: the sequence's k kept positions of this (layer, head).  The result is clamped
// to the bound: no address follows a value read from memory any further.
__device__ __forceinline__ int ragged_src_row(const RaggedRule& r, const RaggedSeq& s, const int32_t* idx_row, int row) {
  if (!s.pruned || row < r.start) return row;
  const int j = row < r.start + r.k ? idx_row[row - r.start] : s.hi + (row - r.start - r.k);
  return min(max(j, 0), r.bound - 1);
}

template <typename T>
struct RaggedSelectParams {
  RaggedRule rule;
  const void* const* score_ptrs; int64_t score_sb, score_sh;
  int32_t* idx;                    // [layers, B, H, k]
  int32_t* new_lens;               // [B]
};

// one workgroup per (layer, sequence, head); VPT == 0: the radix select of select_row.h (windows beyond 32768 scores)
template <typename T, int NT, int VPT>
__global__ __launch_bounds__(NT) void prune_ragged_select_kernel(const RaggedSelectParams<T> p) {
  const RaggedRule& r = p.rule;
  const int h = blockIdx.x % r.H, lb = blockIdx.x / r.H, b = lb % r.B, layer = lb / r.B;
  const RaggedSeq s = ragged_seq(r, b);
  if (lb == b && h == 0 && threadIdx.x == 0) p.new_lens[b] = s.new_len;      // layer 0
  if (!s.pruned) return;                                                     // (uniform) its idx rows are left untouched
  const T* const row0 = (const T*)p.score_ptrs[layer] + b * p.score_sb + h * p.score_sh + r.start;
  int32_t* const out0 = p.idx + (int64_t)blockIdx.x * r.k;
  const int W0 = s.hi - r.start;             // k < W0 <= bound - start
  if constexpr (VPT == 0) {
    topk_select_row<T>(row0, W0, r.k, r.start, out0);
  } else {
    const struct { int lo, k; } p = {r.start, r.k};      // (what the included body reads of its kernel's block)
#define SEL_WINDOW const T* row = row0; int32_t* out = out0; const int W = W0;
#include "select_reg_body.inc"
#undef SEL_WINDOW
  }
}

struct RaggedCompactParams {
  RaggedRule rule;
  const void* const* k_src_ptrs; const void* const* v_src_ptrs;
  void* const* k_dst_ptrs; void* const* v_dst_ptrs; void* const* kr_dst_ptrs;
  const void* cos; const void* sin; int table_rows;
  int64_t src_sb, src_sh, dst_sb, dst_sh;   // in BYTES
  const int32_t* idx;
  int out_rows, ppr, row_bytes, hp_shift, rows_per_block;   // as in kv_compact_kernel (prune.hip)
};

// kv_compact_kernel's mapping — one lane per PAIR of 16-byte pieces (pc, pc + ppr/2) of a destination row, grid = (row blocks,
// B * H, layers * 2) — over rows [0, out_rows): rows below the sequence's new length come through its row map, the rest is zero.
template <typename T>
__global__ __launch_bounds__(256) void prune_ragged_compact_kernel(const RaggedCompactParams p) {
  const RaggedRule& rl = p.rule;
  const int half_ppr = p.ppr >> 1;
  const int half_bytes = p.row_bytes >> 1;
  int piece, rloc;
  if (p.hp_shift >= 0) { piece = threadIdx.x & (half_ppr - 1); rloc = threadIdx.x >> p.hp_shift; }
  else { rloc = threadIdx.x / half_ppr; piece = threadIdx.x - rloc * half_ppr; }
  const int r = blockIdx.x * p.rows_per_block + rloc;
  if (rloc >= p.rows_per_block || r >= p.out_rows) return;
  const int bh = blockIdx.y, b = bh / rl.H, h = bh - b * rl.H;                    // wave-uniform
  const int layer = blockIdx.z >> 1, t = blockIdx.z & 1;
  const bool want_kr = t == 0 && p.kr_dst_ptrs != nullptr;
  const RaggedSeq s = ragged_seq(rl, b);
  char* dbase = (char*)(t == 0 ? p.k_dst_ptrs[layer] : p.v_dst_ptrs[layer]);
  const int64_t doff = b * p.dst_sb + h * p.dst_sh + (int64_t)r * p.row_bytes + piece * 16;
  char* rbase = want_kr ? (char*)p.kr_dst_ptrs[layer] : nullptr;
  if (r >= s.new_len) {                      // past the sequence's new length: the defined region is zero
    const u32x4 zero = {0u, 0u, 0u, 0u};
    __builtin_nontemporal_store(zero, reinterpret_cast<u32x4*>(dbase + doff));
    __builtin_nontemporal_store(zero, reinterpret_cast<u32x4*>(dbase + doff + half_bytes));
    if (want_kr) {
      __builtin_nontemporal_store(zero, reinterpret_cast<u32x4*>(rbase + doff));
      __builtin_nontemporal_store(zero, reinterpret_cast<u32x4*>(rbase + doff + half_bytes));
    }
    return;
  }
  const int src_row = ragged_src_row(rl, s, p.idx + ((int64_t)(layer * rl.B + b) * rl.H + h) * rl.k, r);
  const char* sbase = (const char*)(t == 0 ? p.k_src_ptrs[layer] : p.v_src_ptrs[layer]);
  const char* sp = sbase + b * p.src_sb + h * p.src_sh + (int64_t)src_row * p.row_bytes + piece * 16;
  const u32x4 lo_v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(sp));
  const u32x4 hi_v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(sp + half_bytes));
  u32x4 cs, sn;
  if (want_kr) {
    const int pos = min(r, p.table_rows - 1);
    const int64_t toff = (int64_t)pos * half_bytes + piece * 16;
    cs = *reinterpret_cast<const u32x4*>((const char*)p.cos + toff);
    sn = *reinterpret_cast<const u32x4*>((const char*)p.sin + toff);
  }
  __builtin_nontemporal_store(lo_v, reinterpret_cast<u32x4*>(dbase + doff));
  __builtin_nontemporal_store(hi_v, reinterpret_cast<u32x4*>(dbase + doff + half_bytes));
  if (want_kr) {
#include "rope_piece_pair.inc"
  }
}

// all layers' fp32 accumulators through the same row maps: grid = (column blocks, B * acc_heads, layers); accumulator row a
// follows KV head a / group
__global__ __launch_bounds__(256) void prune_ragged_acc_kernel(const RaggedRule rl, const float* const* __restrict__ src_ptrs,
                                                               int64_t src_sb, int64_t src_sh, float* const* __restrict__ dst_ptrs,
                                                               int64_t dst_sb, int64_t dst_sh, const int32_t* __restrict__ idx,
                                                               int acc_heads, int group, int acc_cols) {
  const int c = blockIdx.x * 256 + threadIdx.x, ba = blockIdx.y, b = ba / acc_heads, a = ba - b * acc_heads, l = blockIdx.z;
  if (c >= acc_cols) return;
  const RaggedSeq s = ragged_seq(rl, b);
  float v = 0.f;
  if (c < s.new_len) {
    const int j = ragged_src_row(rl, s, idx + ((int64_t)(l * rl.B + b) * rl.H + a / group) * rl.k, c);
    v = src_ptrs[l][b * src_sb + a * src_sh + j];
  }
  dst_ptrs[l][b * dst_sb + a * dst_sh + c] = v;
}

template <typename T>
static int launch_ragged_select(const RaggedSelectParams<T>& p, int layers, hipStream_t st) {
  const RaggedRule& r = p.rule;
  const int W = r.bound - r.start;            // the longest window any sequence can have
  const int rows = layers * r.B * r.H;
  const dim3 grid((unsigned)rows);
  const bool many = rows >= 128;              // prune.hip's launch_select rule: many windows -> 4-wave workgroups
#define SPATTEN_RSEL(NT_, VPT_) hipLaunchKernelGGL((prune_ragged_select_kernel<T, NT_, VPT_>), grid, dim3(NT_), 0, st, p)
  if (W > 32768) SPATTEN_RSEL(kSelThreads, 0);
  else if (W <= 1024) SPATTEN_RSEL(256, 4);
  else if (many && W <= 4096) SPATTEN_RSEL(256, 16);
  else if (many && W <= 8192) SPATTEN_RSEL(256, 32);
  else if (W <= 4096) SPATTEN_RSEL(1024, 4);
  else if (W <= 16384) SPATTEN_RSEL(1024, 16);
  else SPATTEN_RSEL(1024, 32);
#undef SPATTEN_RSEL
  return hipGetLastError() == hipSuccess ? SPATTEN_OK : SPATTEN_ERR_LAUNCH;
}

}  // namespace spatten

using namespace spatten;

extern "C" int spatten_prune_ragged(const spatten_prune_ragged_args_t* a, void* stream) {
  // ---- every refusal is host arithmetic before the first launch ----
  if (!a || a->struct_size != sizeof(spatten_prune_ragged_args_t)) return SPATTEN_ERR_INVALID;
  if (!ok_dtype(a->score_dtype) || !ok_dtype(a->kv_dtype)) return SPATTEN_ERR_INVALID;
  if (!a->lens || !a->score_ptrs || !a->k_src_ptrs || !a->v_src_ptrs || !a->k_dst_ptrs || !a->v_dst_ptrs || !a->idx || !a->new_lens)
    return SPATTEN_ERR_INVALID;
  if (a->layers <= 0 || a->batch <= 0 || a->heads <= 0 || a->head_dim <= 0 || a->lens_step <= 0 || a->bound <= 0) return SPATTEN_ERR_INVALID;
  // (a window shorter than k cannot be reported from the device: the rule below makes every pruned window longer than k)
  if (a->start < 0 || a->k <= 0 || a->recent < 0 || a->num_coming < 0 || a->num_coming > a->recent) return SPATTEN_ERR_INVALID;
  const long long keep_ll = (long long)a->start + a->k + a->recent - a->num_coming;
  if (keep_ll > 0x7FFFFFFFll - a->recent || a->out_rows < keep_ll) return SPATTEN_ERR_INVALID;
  const int keep_rows = (int)keep_ll;
  if (a->score_batch_stride < 0 || a->score_head_stride < 0 || a->src_batch_stride < 0 || a->src_head_stride < 0 ||
      a->dst_batch_stride < 0 || a->dst_head_stride < 0)
    return SPATTEN_ERR_INVALID;
  if (a->kr_dst_ptrs && (!a->cos || !a->sin || a->table_rows < a->out_rows)) return SPATTEN_ERR_INVALID;
  if ((a->acc_src_ptrs == nullptr) != (a->acc_dst_ptrs == nullptr)) return SPATTEN_ERR_INVALID;
  if (a->acc_src_ptrs) {
    if (a->acc_heads <= 0 || a->acc_heads % a->heads != 0 || a->acc_cols < keep_rows) return SPATTEN_ERR_INVALID;
    if (a->acc_src_batch_stride < 0 || a->acc_src_head_stride < 0 || a->acc_dst_batch_stride < 0 || a->acc_dst_head_stride < 0)
      return SPATTEN_ERR_INVALID;
  }
  const int es = a->kv_dtype == SPATTEN_F32 ? 4 : 2;
  const long long row_bytes = (long long)a->head_dim * es;
  if (row_bytes % 32 != 0 || row_bytes / 32 > 256) return SPATTEN_ERR_UNSUPPORTED;      // rows move as pairs of 16-byte pieces
  const int half_ppr = (int)(row_bytes / 32);
  const int rows_per_block = 256 / half_ppr;
  const long long sel_rows = (long long)a->layers * a->batch * a->heads;
  const long long grid_y = (long long)a->batch * a->heads, grid_z = (long long)a->layers * 2;
  if (sel_rows >= (1ll << 31) || sel_rows * a->k >= (1ll << 40) || grid_y > 65535 || grid_z > 65535) return SPATTEN_ERR_UNSUPPORTED;
  if (a->acc_src_ptrs && (long long)a->batch * a->acc_heads > 65535) return SPATTEN_ERR_UNSUPPORTED;

  hipStream_t st = (hipStream_t)stream;
  RaggedRule rule;
  rule.lens = a->lens; rule.lens_step = a->lens_step;
  rule.bound = a->bound; rule.start = a->start; rule.recent = a->recent; rule.k = a->k; rule.num_coming = a->num_coming;
  rule.B = a->batch; rule.H = a->heads;

  // 1. select (and the new lengths)
  int rc;
#define SPATTEN_RAGGED_SELECT(T)                                                                         \
  {                                                                                                      \
    RaggedSelectParams<T> sp;                                                                            \
    sp.rule = rule; sp.score_ptrs = a->score_ptrs; sp.score_sb = a->score_batch_stride; sp.score_sh = a->score_head_stride; \
    sp.idx = a->idx; sp.new_lens = a->new_lens;                                                          \
    rc = launch_ragged_select<T>(sp, a->layers, st);                                                     \
  }
  switch (a->score_dtype) {
    case SPATTEN_F32: SPATTEN_RAGGED_SELECT(float) break;
    case SPATTEN_F16: SPATTEN_RAGGED_SELECT(f16_t) break;
    default: SPATTEN_RAGGED_SELECT(bf16_t)
  }
#undef SPATTEN_RAGGED_SELECT
  if (rc != SPATTEN_OK) return rc;

  // 2. K / V rows + the rotated shadow
  RaggedCompactParams cp;
  cp.rule = rule;
  cp.k_src_ptrs = a->k_src_ptrs; cp.v_src_ptrs = a->v_src_ptrs; cp.k_dst_ptrs = a->k_dst_ptrs; cp.v_dst_ptrs = a->v_dst_ptrs;
  cp.kr_dst_ptrs = a->kr_dst_ptrs; cp.cos = a->cos; cp.sin = a->sin; cp.table_rows = a->table_rows;
  cp.src_sb = a->src_batch_stride * es; cp.src_sh = a->src_head_stride * es;
  cp.dst_sb = a->dst_batch_stride * es; cp.dst_sh = a->dst_head_stride * es;
  cp.idx = a->idx; cp.out_rows = a->out_rows; cp.ppr = 2 * half_ppr; cp.row_bytes = (int)row_bytes;
  cp.hp_shift = -1;
  for (int sft = 0; sft < 9; ++sft) if ((1 << sft) == half_ppr) cp.hp_shift = sft;
  cp.rows_per_block = rows_per_block;
  {
    const dim3 grid((unsigned)ceil_div(a->out_rows, rows_per_block), (unsigned)grid_y, (unsigned)grid_z);
    SPATTEN_BY_DTYPE(a->kv_dtype, hipLaunchKernelGGL((prune_ragged_compact_kernel<T>), grid, dim3(256), 0, st, cp));
    if (hipGetLastError() != hipSuccess) return SPATTEN_ERR_LAUNCH;
  }

  // 3. the accumulators through the same row maps
  if (a->acc_src_ptrs) {
    const dim3 grid((unsigned)ceil_div(a->acc_cols, 256), (unsigned)(a->batch * a->acc_heads), (unsigned)a->layers);
    hipLaunchKernelGGL(prune_ragged_acc_kernel, grid, dim3(256), 0, st, rule, a->acc_src_ptrs, a->acc_src_batch_stride,
                       a->acc_src_head_stride, a->acc_dst_ptrs, a->acc_dst_batch_stride, a->acc_dst_head_stride, a->idx, a->acc_heads,
                       a->acc_heads / a->heads, a->acc_cols);
    if (hipGetLastError() != hipSuccess) return SPATTEN_ERR_LAUNCH;
  }
  return SPATTEN_OK;
}
