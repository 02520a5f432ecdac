// pq_gqa.hip — the MSB pass of the quantised-query decode over the profiled planes for a GROUPED-QUERY model, on the int8 matrix
// cores (include/spatten.h "Grouped quantised-query decode"; opt-in: spatten_attn_decode_pq_qint_gqa).  PARITY UNPINNED, as the
// per-query-head form (pq_decode.hip).
//
// pq_decode.hip launches one workgroup column per QUERY head: the G = H / Hkv heads of a group each fetch their kv head's MSB,
// scale and value planes and each redo the field arithmetic on them.  Here a workgroup column is a KV head (decode_gqa.hip's
// shape): a row's bytes are touched once per group and scored for all G heads with
//     S^T = Kmsb · Qint^T   (32 keys x 32 columns per v_mfma_i32_32x32x32_i8; the group's quantised queries are the first G columns,
//                            columns >= G are zeros; the plane stores msb + 128: the signed operand is the byte XOR 0x80)
//     O^T = Vt · W^T        (v_mfma_f32_32x32x16_bf16 for BOTH model dtypes: an 8-bit qv is exact in bf16; the weight
//                            w_j = p_j val_scale_j (fp32) enters as hi + lo, hi = bf16(w), lo = bf16(w - hi): two products)
// The plane rows are in PIECE order and are used as they lie: the int8 dot does not care about the order of its 128 terms as long
// as the query operand is permuted the same way (lane (column, half) holds pieces 2 kk + half of its head's query, kk = 0..3, next
// to the 16 bytes at 16 (2 kk + half) of a key row); the exported q_int is in ELEMENT order.  Operand layout of the 32x32x32 int8
// form (checked with exact integer data: tools/mb/mfma_i8_map.hip): lane l holds index l & 31 and the 16 k-bytes 16 (l >> 5) .. +16
// of the 32; the accumulator layout is the 32x32 fp32 one (mfma_tiles.h).
// The value bytes need the key as the contraction index.  Lane (m, half) reads dword m of 8 rows of the tile (one d-quad of 8 keys,
// ds_read_b32: 32 lanes = one 128-byte row, no bank conflict) and turns byte j of each into the bf16 A operand of product j: the
// row index m of product j IS plane byte 4 m + j — the output comes out in plane-byte order and is put into element order once,
// when it is stored.
//
// Mapping: grid = (S splits, Hkv, B), 256 threads = 4 waves; a split's 32-row tiles go round-robin to the waves, which never
// synchronise inside the stream: every wave has a private ring of kStages stages { K tile 4 KiB, V tile 4 KiB, key_scale, val_scale }
// filled by LDS-DMA, refilled with the tile kStages ahead as soon as a stage is consumed.  A split's chunk is at least one tile per
// wave.  The query quantisation is pq_qint.h's (the routine the per-query-head kernels use), the scale chain is the header's to
// the letter — msb_logit, the MSB-only stash, q_int and q_scale are bit-identical to spatten_attn_decode_pq_qint's.  Split
// partials ({value, tag} granules) and the merge are the decode family's (decode_body.h) on the shared workspace.  The refetch
// pass is pq_decode.hip's compact pass 2, launched behind this kernel.
#include <stdlib.h>

#include <algorithm>

#include "common.h"
#include "decode_body.h"
#include "mfma_tiles.h"
#include "pq_qint.h"

namespace spatten {

template <typename T>
struct PqGqaParams {
  const T* q; int64_t q_sb, q_sh;
  PlanesDev pl;
  const T* cos; const T* sin; int table_rows, pos_q;
  const int32_t* step;                                      // device-length form: word 0 = the live length (N is then the bound)
  T* out; int64_t out_sb;
  T* scores; int64_t sc_sb, sc_sh; int sc_vec;              // sc_vec: stash rows 8-byte aligned -> four logits per store
  int lg_vec;                                               // msb_logit rows 16-byte aligned -> four logits per store
  float* lse; int32_t* need; float thr;
  int8_t* qi_out; int64_t qi_sb, qi_sh; float* qs_out; int qmax;
  unsigned* ws_err; unsigned* ws_cnt; unsigned long long* ws_part; int64_t ws_unit;
  int B, H, Hkv, G, N, S, chunk, poll_merge;
  float sqrt_d;
};

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int kPqGqaStages = 3;

// s_waitcnt vmcnt(n) only (gfx9 encoding: vmcnt in bits 3:0 and 15:14; expcnt / lgkmcnt left at "no wait")
template <int N> __device__ inline void pqg_wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt");
  __builtin_amdgcn_s_waitcnt(0x0F70 | (N & 15) | ((N >> 4) << 14));
}
// the element (of the head's d = 128) that byte `pos` of a piece-ordered plane row holds (include/spatten.h "Plane layouts")
__device__ inline int pqg_elem_of(int pos) {
  const int c = pos >> 4, t = pos & 15;
  return t < 8 ? 8 * c + t : 64 + 8 * c + (t - 8);
}

template <typename T, bool DYN>
__global__ __launch_bounds__(256, 1) void pq_gqa_kernel(const PqGqaParams<T> p) {
  constexpr int D = 128, KT = 32, NW = 4, NS = kPqGqaStages;
  constexpr int KBYTES = KT * D;                      // a tile's MSB-plane rows (4 KiB); as many value-plane bytes
  constexpr int SCB = 256;                            // a tile's row scales as one dword DMA (lanes >= 32 fetch nothing: zeros)
  constexpr int STAGE = 2 * KBYTES + 2 * SCB, WBUF = NS * STAGE;
  constexpr int NK = KBYTES / 1024;                   // 16-byte DMA instructions per tile and plane
  constexpr int NREQ = 2 * NK + 2;                    // requests per tile
  constexpr int PITCH = D + 4;                        // floats per (wave, column) partial in LDS: o[D] (plane-byte order), m, l
  static_assert(32 * PITCH * 4 <= WBUF, "a wave's partials fit its ring");
  using V8 = Vec8<T>;
  using raw_t = typename V8::raw;
  using bfrag = typename Mfma<bf16_t>::frag;
  __shared__ __attribute__((aligned(1024))) char lds[NW * WBUF];
  __shared__ unsigned s_gen[32];
  __shared__ unsigned s_ticket;

  const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int split = blockIdx.x, hkv = blockIdx.y, b = blockIdx.z;
  const int G = p.G;
  const int unit0 = b * p.H + hkv * G;                // the group's first softmax row (workspace index of head hkv * G)
  const int lo = split * p.chunk;
  char* const wbuf = lds + wave * WBUF;

  int n_live = p.N;
  if (DYN) n_live = p.step[0];

  // ---- the group's rotated queries: lane (col, hi) holds pieces c = 2 kk + hi of head hkv G + min(col, G - 1) -----------------
  raw_t q_raw[4][4];
  {
    const int gq = min(col, G - 1);
    const T* qrow = p.q + b * p.q_sb + (int64_t)(hkv * G + gq) * p.q_sh;
    const int ps = min(max(p.pos_q, 0), p.table_rows - 1);
    const T* cr = p.cos + (int64_t)ps * (D / 2);
    const T* sr = p.sin + (int64_t)ps * (D / 2);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int c = 2 * kk + hi;
      q_raw[kk][0] = V8::ldg(qrow + 8 * c);
      q_raw[kk][1] = V8::ldg(qrow + D / 2 + 8 * c);
      q_raw[kk][2] = V8::ldg(cr + 8 * c);
      q_raw[kk][3] = V8::ldg(sr + 8 * c);
    }
  }
  // launch generations of the group's units (tags of the partials), parked in LDS for the publish / merge loops
  if (p.S > 1 && tid < G) s_gen[tid] = p.ws_cnt[2 * (unit0 + tid) + 1];

  const int N = DYN ? min(__builtin_amdgcn_readfirstlane(n_live), p.N) : p.N;
  const int hi_all = min(lo + p.chunk, N);
  const int nt = hi_all > lo ? (hi_all - lo + KT - 1) / KT : 0;      // tiles of this split that hold a live row

  // ---- the ring: buffer descriptors end at the planes' bound (rows past it read as zeros without touching memory) ----------------
  auto rsrc_of = [&](const void* base, int64_t bytes) {
    const uint64_t a = (uint64_t)base;
    return i32x4{(int)__builtin_amdgcn_readfirstlane((uint32_t)a), (int)__builtin_amdgcn_readfirstlane((uint32_t)(a >> 32) & 0xFFFFu),
                 (int)(bytes < 0x7FFFFFFF ? bytes : 0x7FFFFFFF), 0x00020000};
  };
  const i32x4 k_rsrc = rsrc_of(p.pl.km + b * p.pl.km_sb + hkv * p.pl.km_sh, (int64_t)p.N * D);
  const i32x4 v_rsrc = rsrc_of(p.pl.vq + b * p.pl.vq_sb + hkv * p.pl.vq_sh, (int64_t)p.N * D);
  const i32x4 ks_rsrc = rsrc_of(p.pl.ks + b * p.pl.sc_sb + hkv * p.pl.sc_sh, (int64_t)p.N * 4);
  const i32x4 vs_rsrc = rsrc_of(p.pl.vs + b * p.pl.sc_sb + hkv * p.pl.sc_sh, (int64_t)p.N * 4);
  const unsigned lds_wbuf = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)lds + (unsigned)wave * WBUF;
  // The requests are inline assembly (decode_gqa.hip: behind the compiler's own LDS-DMA builtin every later LDS read waits for
  // vmcnt(0), i.e. for the tiles requested a moment ago as well).  Non-temporal: every plane byte is used once per launch.
  auto dma16a = [&](const i32x4& rsrc, unsigned lds_dst, int voff, int soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen nt lds"
                 :: "s"(lds_dst), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
  };
  auto dma4a = [&](const i32x4& rsrc, unsigned lds_dst, int voff, int soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %3 offen nt lds"
                 :: "s"(lds_dst), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
  };
  // A 1-KiB DMA piece is 8 plane rows.  Keys: lane (row-in-piece lr, physical 16-byte slot ps) fetches logical slot ps ^ lr, so
  // that the 32 rows' A-operand reads (ds_read_b128, one slot per row) spread over the banks; values stay row-major.
  auto dma_tile = [&](int tile, int stage) {
    const int ln = opaque_lane(lane);
    const int lr = ln >> 3, ps = ln & 7;
    const int kvo = lr * 128 + ((ps ^ lr) << 4), vvo = ln * 16;
    const int svo = ln < 32 ? ln * 4 : 0x40000000;    // (beyond every descriptor: a zero, no memory access)
    const unsigned st = lds_wbuf + stage * STAGE;
    const int row0 = lo + tile * KT;
    const int soff = __builtin_amdgcn_readfirstlane(row0 * D), soff_s = __builtin_amdgcn_readfirstlane(row0 * 4);
    dma4a(ks_rsrc, st + 2 * KBYTES, svo, soff_s);
#pragma unroll
    for (int i = 0; i < NK; ++i) dma16a(k_rsrc, st + i * 1024, kvo, soff + i * 1024);
    dma4a(vs_rsrc, st + 2 * KBYTES + SCB, svo, soff_s);
#pragma unroll
    for (int i = 0; i < NK; ++i) dma16a(v_rsrc, st + KBYTES + i * 1024, vvo, soff + i * 1024);
  };
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int s = 0; s < NS; ++s)
    if (wave + s * NW < nt) dma_tile(wave + s * NW, s);
  __builtin_amdgcn_sched_barrier(0);

  // ---- rotate (modify_llama.py:92), quantise (pq_qint.h) and pack the queries as B operands; split 0 exports them ----------------
  i32x4 qb[4];
  float cq;
  const float rsqrt_d = 1.0f / p.sqrt_d;
  {
    float qv[4][16];
    float amax = 0.f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      float xlo[8], xhi[8], cc[8], ss[8], ylo[8], yhi[8];
      V8::unpack(q_raw[kk][0], xlo);
      V8::unpack(q_raw[kk][1], xhi);
      V8::unpack(q_raw[kk][2], cc);
      V8::unpack(q_raw[kk][3], ss);
      rope_pair<T>(xlo, xhi, cc, ss, ylo, yhi);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        qv[kk][i] = ylo[i]; qv[kk][8 + i] = yhi[i];
        amax = fmaxf(amax, fmaxf(fabsf(ylo[i]), fabsf(yhi[i])));
      }
    }
    amax = xor32_max(amax);                           // (a maximum: exact in any order — the head's, as the per-head kernels')
    const float qmaxf = (float)p.qmax;
    float qs, qs_div;
    qint_scale(amax, qmaxf, qs, qs_div);
    cq = qs * (16.f * rsqrt_d);
    const bool live = col < G;
    const bool exporter = live && split == 0;
    int8_t* qrow_out = p.qi_out + b * p.qi_sb + (int64_t)(hkv * G + min(col, G - 1)) * p.qi_sh;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      int qi[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) qi[t] = qint_round(qv[kk][t], qs_div, qmaxf);
      uint32_t w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = pack_i8x4(qi[4 * j], qi[4 * j + 1], qi[4 * j + 2], qi[4 * j + 3]);
      if (exporter) {                                 // element order: elements 8c .. 8c + 7 and d/2 + 8c ..
        const int c = 2 * kk + hi;
        *reinterpret_cast<u32x2*>(qrow_out + 8 * c) = u32x2{w[0], w[1]};
        *reinterpret_cast<u32x2*>(qrow_out + D / 2 + 8 * c) = u32x2{w[2], w[3]};
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) qb[kk][j] = live ? (int)w[j] : 0;
    }
    if (exporter && hi == 0) p.qs_out[unit0 + col] = qs;
  }

  T* stashp = (p.scores != nullptr && col < G) ? p.scores + b * p.sc_sb + (int64_t)(hkv * G + col) * p.sc_sh : nullptr;
  float* lgp = col < G ? p.pl.lg + b * p.pl.lg_sb + (int64_t)(hkv * G + col) * p.pl.lg_sh : nullptr;
  float m_run = -INFINITY, l_run = 0.f;
  f32x16 o[4];                                        // product j: rows = plane bytes 4 m + j
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[j][r] = 0.f;

  const unsigned lds0 = (unsigned)(wbuf - lds);
  for (int i = wave, k = 0; i < nt; i += NW, ++k) {
    const int stage = k % NS;
    const int row0 = lo + i * KT;
    // loads return in order: "at most X outstanding" with X = the requests of the tiles issued behind this one proves it has landed
    // whatever the stores in between do (they may only make the wait longer)
    const int behind = min(NS - 1, (nt - 1 - i) / NW);
    if (behind >= 2) pqg_wait_vm<2 * NREQ>(); else if (behind == 1) pqg_wait_vm<NREQ>(); else pqg_wait_vm<0>();
    static_assert(NS == 3, "the waits above are written out for three stages");
    __builtin_amdgcn_sched_barrier(0);

    // ---- S^T = Kmsb · Qint^T: exact int32 ---------------------------------------------------------------------------------------
    i32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0;
    {
      const unsigned ku = lds0 + stage * STAGE + col * 128;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        u32x4 a = *reinterpret_cast<const u32x4*>(lds + ku + ((((unsigned)(2 * kk + hi)) ^ ((unsigned)col & 7u)) << 4));
        a ^= 0x80808080u;                              // stored msb + 128 -> msb (two's complement)
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(*reinterpret_cast<const i32x4*>(&a), qb[kk], acc, 0, 0, 0);
      }
    }
    // s1 = float(A1) (key_scale cq): register r is key row0 + (r & 3) + 8 (r >> 2) + 4 hi
    const float* ksl = reinterpret_cast<const float*>(lds + lds0 + stage * STAGE + 2 * KBYTES);
    const float* vsl = reinterpret_cast<const float*>(lds + lds0 + stage * STAGE + 2 * KBYTES + SCB);
    float s[16], vsc[16];
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const f32x4 k4 = *reinterpret_cast<const f32x4*>(ksl + 8 * q4 + 4 * hi);
      const f32x4 v4 = *reinterpret_cast<const f32x4*>(vsl + 8 * q4 + 4 * hi);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s[4 * q4 + e] = (float)acc[4 * q4 + e] * (k4[e] * cq);
        vsc[4 * q4 + e] = v4[e];
      }
    }
    // msb_logit (fp32) and the stash (model dtype): four consecutive keys per store where the rows are aligned and whole
    if (col < G) {
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int key = row0 + 8 * q4 + 4 * hi;
        if (p.lg_vec && key + 3 < N) {
          *reinterpret_cast<f32x4*>(lgp + key) = f32x4{s[4 * q4], s[4 * q4 + 1], s[4 * q4 + 2], s[4 * q4 + 3]};
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (key + e < N) lgp[key + e] = s[4 * q4 + e];
        }
        if (stashp == nullptr) continue;
        if (p.sc_vec && key + 3 < N) {
          typedef T t4 __attribute__((ext_vector_type(4)));
          t4 pk;
#pragma unroll
          for (int e = 0; e < 4; ++e) pk[e] = DT<T>::from_f32(s[4 * q4 + e]);
          *reinterpret_cast<t4*>(stashp + key) = pk;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (key + e < N) stashp[key + e] = DT<T>::from_f32(s[4 * q4 + e]);
        }
      }
    }
    if (row0 + KT > N) {                               // (a select, not arithmetic: a dead row's scales may be anything)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = row0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        s[r] = key < N ? s[r] : -INFINITY;
      }
    }
    // ---- online softmax of the column (lanes col and col + 32 hold its 32 keys) -------------------------------------------------
    float mt = fmaxf(s[0], s[1]);
#pragma unroll
    for (int r = 2; r < 16; r += 2) mt = fmaxf(mt, fmaxf(s[r], s[r + 1]));
    mt = xor32_max(mt);
    const float m_new = fmaxf(m_run, mt);
    const float mu = (m_new == -INFINITY) ? 0.f : m_new;
    if (m_new > m_run) {                               // the first tile; rare afterwards
      const float alpha = __expf(m_run - mu);          // m_run = -inf -> 0
      l_run *= alpha;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[j][r] *= alpha;
      m_run = m_new;
    }
    // the weights w = p val_scale (fp32) as hi + lo bf16 B operands: fragment t, element e = register 8 t + e
    bfrag wh[2], wl[2];
    {
      float ls[2] = {0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float sv = s[8 * t + e];
          const float pv = sv == -INFINITY ? 0.f : __expf(sv - mu);
          ls[e & 1] += pv;
          const float w = sv == -INFINITY ? 0.f : pv * vsc[8 * t + e];
          const bf16_t h = (bf16_t)w;
          wh[t][e] = h;
          wl[t][e] = (bf16_t)(w - (float)h);
        }
      l_run += ls[0] + ls[1];
    }
    // ---- O^T += Vt · W^T ---------------------------------------------------------------------------------------------------------
    {
      const unsigned vu = lds0 + stage * STAGE + KBYTES + 4 * col;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        uint32_t dw[8];                                // element e: key 16 t + 4 hi + (e & 3) + 8 (e >> 2), this lane's d-quad
#pragma unroll
        for (int e = 0; e < 8; ++e)
          dw[e] = *reinterpret_cast<const uint32_t*>(lds + vu + (16 * t + 4 * hi + (e & 3) + 8 * (e >> 2)) * D);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          union { uint32_t u[4]; bfrag f; } a;
#pragma unroll
          for (int e = 0; e < 8; e += 2) {
            // qv = byte - 128, exact in fp32 and in bf16: the bf16 IS the upper half of the fp32
            const float f0 = (float)((dw[e] >> (8 * j)) & 255u) - 128.f, f1 = (float)((dw[e + 1] >> (8 * j)) & 255u) - 128.f;
            a.u[e / 2] = __builtin_amdgcn_perm(__float_as_uint(f1), __float_as_uint(f0), 0x07060302u);
          }
          o[j] = Mfma<bf16_t>::mma(a.f, wh[t], o[j]);
          o[j] = Mfma<bf16_t>::mma(a.f, wl[t], o[j]);
        }
      }
    }
    // the stage is consumed (its last read fed the last product): request the tile NS ahead into it
    __builtin_amdgcn_sched_barrier(0);
    if (i + NS * NW < nt) dma_tile(i + NS * NW, stage);
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- the four waves' partials -> LDS (each wave into its own ring: all its requests have landed and been consumed) -------------
  {
    pqg_wait_vm<0>();
    const float l_col = xor32_sum(l_run);
    float* part = reinterpret_cast<float*>(wbuf);
    if (col < G) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int mrow = (r & 3) + 8 * (r >> 2) + 4 * hi;            // plane bytes 4 mrow .. + 3
        *reinterpret_cast<f32x4*>(part + col * PITCH + 4 * mrow) = f32x4{o[0][r], o[1][r], o[2][r], o[3][r]};
      }
      if (hi == 0) { part[col * PITCH + D] = m_run; part[col * PITCH + D + 1] = l_col; }
    }
  }
  __syncthreads();

  // ---- fold the waves, publish the split's partial per head (granule e = plane byte e: this kernel's own order) -------------------
  const int items = G * D;
  for (int idx = tid; idx < items; idx += 256) {
    const int g = idx >> 7, e = idx & (D - 1);
    float mw[NW], mwg = -INFINITY;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      mw[w] = reinterpret_cast<const float*>(lds + w * WBUF)[g * PITCH + D];
      mwg = fmaxf(mwg, mw[w]);
    }
    const float mu = (mwg == -INFINITY) ? 0.f : mwg;
    float o_tot = 0.f, l_tot = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float* pw = reinterpret_cast<const float*>(lds + w * WBUF) + g * PITCH;
      const float ww = __expf(mw[w] - mu);            // exp(-inf) = 0: a wave without tiles
      o_tot = fmaf(pw[e], ww, o_tot);
      l_tot = fmaf(pw[D + 1], ww, l_tot);
    }
    const int unit = unit0 + g;
    if (p.S == 1) {
      p.out[b * p.out_sb + (int64_t)(hkv * G + g) * D + pqg_elem_of(e)] = DT<T>::from_f32(o_tot / l_tot);
      if (e == 0) {
        if (p.lse != nullptr) { p.lse[2 * unit] = mwg; p.lse[2 * unit + 1] = l_tot; }
        p.need[unit] = (1.0f / l_tot) < p.thr ? 1 : 0;            // max prob = exp(0) / sum
      }
      continue;
    }
    unsigned long long* part = p.ws_part + (int64_t)unit * p.ws_unit + (int64_t)split * (D + 2);
    const unsigned tag = (s_gen[g] & 0x7FFFFFFFu) + 1u;
    store_granule(part + e, o_tot, tag);
    if (e == 0) { store_granule(part + D, mwg, tag); store_granule(part + D + 1, l_tot, tag); }
  }
  if (p.S == 1) return;

  // ---- merge (decode_gqa.hip): with the whole grid co-resident (poll_merge) the workgroup of split S-1 - g % S polls for head g's
  // granules — the G heads of a group are merged by G different workgroups at once; otherwise the group's last ARRIVER merges all
  if (!p.poll_merge) {
    __syncthreads();
    if (tid == 0) s_ticket = __hip_atomic_fetch_add(p.ws_cnt + 2 * unit0, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_ticket != (unsigned)(p.S - 1)) return;
  }
  float* const fold = reinterpret_cast<float*>(lds);  // [D][3] of the upper half (the wave partials are dead behind the barrier below)
  constexpr int KB = 16;
  for (int g = 0; g < G; ++g) {
    if (p.poll_merge && split != p.S - 1 - (g % p.S)) continue;          // (workgroup-uniform)
    const int e = tid & (D - 1), half = tid >> 7;
    const int unit = unit0 + g;
    const unsigned long long* ws = p.ws_part + (int64_t)unit * p.ws_unit;
    const unsigned gen = s_gen[g];
    const unsigned tag = (gen & 0x7FFFFFFFu) + 1u;
    float mg = -INFINITY, lg = 0.f, og = 0.f;
    bool expired = false;
    for (int s0 = half; s0 < p.S; s0 += 2 * KB) {
      unsigned long long ga[KB], gm[KB], gl[KB];
      int spins = 0;
      bool landed;
      do {     // every load is issued before any tag is looked at: one round trip per batch
#pragma unroll
        for (int j = 0; j < KB; ++j) {
          const int sc_ = (s0 + 2 * j) < p.S ? (s0 + 2 * j) : s0;
          const unsigned long long* qq = ws + (int64_t)sc_ * (D + 2);
          ga[j] = __hip_atomic_load(qq + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          gm[j] = __hip_atomic_load(qq + D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          gl[j] = __hip_atomic_load(qq + D + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        unsigned diff = 0u;
#pragma unroll
        for (int j = 0; j < KB; ++j)
          diff |= ((unsigned)(ga[j] >> 32) ^ tag) | ((unsigned)(gm[j] >> 32) ^ tag) | ((unsigned)(gl[j] >> 32) ^ tag);
        landed = diff == 0u;
      } while (!landed && ++spins < (1 << 16));       // bounded: a granule that was issued always lands — if not, fail loudly
      expired |= !landed;
      float a[KB], ms[KB], ls[KB];
      float mn = mg;
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        const bool live = (s0 + 2 * j) < p.S;
        a[j] = live ? __uint_as_float((unsigned)ga[j]) : 0.f;
        ms[j] = live ? __uint_as_float((unsigned)gm[j]) : -INFINITY;
        ls[j] = live ? __uint_as_float((unsigned)gl[j]) : 0.f;
        mn = fmaxf(mn, ms[j]);
      }
      const float mu = (mn == -INFINITY) ? 0.f : mn;
      const float w0 = __expf(mg - mu);
      og *= w0; lg *= w0;
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        const float w = __expf(ms[j] - mu);
        og = fmaf(a[j], w, og);
        lg = fmaf(ls[j], w, lg);
      }
      mg = mn;
    }
    if (expired) {   // never merge incomplete data silently: flag the workspace and poison this unit's output
      atomicOr(p.ws_err, 1u);
      og = __builtin_nanf("");
    }
    __syncthreads();                                  // the previous user of `fold` (wave partials / the last head) is done
    if (half == 1) { fold[3 * e] = og; fold[3 * e + 1] = mg; fold[3 * e + 2] = lg; }
    __syncthreads();
    if (half == 0) {
      const float m1 = fold[3 * e + 1];
      const float mn = fmaxf(mg, m1);
      const float mu = (mn == -INFINITY) ? 0.f : mn;
      const float w0 = __expf(mg - mu), w1 = __expf(m1 - mu);
      og = fmaf(fold[3 * e], w1, og * w0);
      lg = fmaf(fold[3 * e + 2], w1, lg * w0);
      p.out[b * p.out_sb + (int64_t)(hkv * G + g) * D + pqg_elem_of(e)] = DT<T>::from_f32(og / lg);
      if (e == 0) {
        if (p.lse != nullptr) { p.lse[2 * unit] = mn; p.lse[2 * unit + 1] = lg; }
        p.need[unit] = (1.0f / lg) < p.thr ? 1 : 0;
        p.ws_cnt[2 * unit + 1] = gen + 1u;            // next launch: new tag
      }
    }
  }
  if (!p.poll_merge && tid == 0) __hip_atomic_store(p.ws_cnt + 2 * unit0, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-arm
}

// The split layout (decode_gqa.hip's rule): one workgroup per CU; a split gets at least one tile per wave (128 rows); chunks are
// whole tiles.
static inline void pq_gqa_layout(int cols, int lay, int n_splits, int ws_splits, int& S, int& chunk32) {
  S = n_splits > 0 ? n_splits : std::max(1, coresident_workgroups() / cols);
  S = std::min(S, std::max(1, lay / 128));
  S = std::min(S, std::min(ws_splits, kDecodeMaxSplits));
  const int chunk = (lay + S - 1) / S;
  chunk32 = (chunk + 31) / 32 * 32;
  S = (lay + chunk32 - 1) / chunk32;
}

template <typename T>
static int run_pq_gqa(const spatten_pq_qint_args_t* qa, const PlanesDev& pd, hipStream_t stream) {
  const spatten_pq_decode_args_t* a = &qa->step;
  const int d = a->head_dim, units = a->batch * a->heads, cols = a->batch * a->kv_heads;
  const int ws_splits = a->workspace_splits > 0 ? a->workspace_splits : kDecodeMaxSplits;
  // the split layout follows the LAYOUT length: a static launch laid out for a longer cache decomposes — bit for bit — like the
  // device-length form whose bound is that length
  const int lay = (!a->step_state && a->kv_len_layout > a->kv_len) ? a->kv_len_layout : a->kv_len;
  int S, chunk32;
  pq_gqa_layout(cols, lay, a->n_splits, ws_splits, S, chunk32);
  if (S > 1 && !a->workspace) return SPATTEN_ERR_INVALID;
  PqGqaParams<T> p;
  p.q = (const T*)a->q; p.q_sb = a->q_sb; p.q_sh = a->q_sh;
  p.pl = pd;
  p.cos = (const T*)a->cos; p.sin = (const T*)a->sin; p.table_rows = a->table_rows; p.pos_q = a->pos_q;
  p.step = (const int32_t*)a->step_state;
  if (a->step_state) {   // the state's staged rotary rows stand in for the table: row 0 = the query's position
    p.cos = (const T*)((const char*)a->step_state + kStepHeader);
    p.sin = p.cos + 2 * (d / 2); p.table_rows = 2; p.pos_q = 0;
  }
  p.out = (T*)a->out; p.out_sb = a->out_sb;
  p.scores = (T*)a->scores; p.sc_sb = a->sc_sb; p.sc_sh = a->sc_sh;
  p.sc_vec = (a->scores && (uintptr_t)a->scores % 8 == 0 && a->sc_sb % 4 == 0 && a->sc_sh % 4 == 0) ? 1 : 0;
  p.lg_vec = ((uintptr_t)pd.lg % 16 == 0 && pd.lg_sb % 4 == 0 && pd.lg_sh % 4 == 0) ? 1 : 0;
  p.lse = a->lse; p.need = a->need_lsb; p.thr = a->threshold;
  p.qi_out = qa->q_int; p.qi_sb = qa->qi_sb; p.qi_sh = qa->qi_sh; p.qs_out = qa->q_scale; p.qmax = (1 << (qa->query_bits - 1)) - 1;
  const size_t cnt_bytes = decode_cnt_bytes((size_t)units);
  p.ws_err = (unsigned*)a->workspace;
  p.ws_cnt = a->workspace ? (unsigned*)((char*)a->workspace + kDecodeWsHeader) : nullptr;
  p.ws_part = a->workspace ? (unsigned long long*)((char*)a->workspace + kDecodeWsHeader + cnt_bytes) : nullptr;
  p.ws_unit = (int64_t)ws_splits * (d + 2);
  p.B = a->batch; p.H = a->heads; p.Hkv = a->kv_heads; p.G = a->heads / a->kv_heads; p.N = a->kv_len; p.S = S; p.chunk = chunk32;
  p.poll_merge = (S > 1 && (long long)S * cols <= coresident_workgroups()) ? 1 : 0;
  p.sqrt_d = sqrtf((float)d);
  const dim3 grid((unsigned)S, (unsigned)a->kv_heads, (unsigned)a->batch);
  if (a->step_state) hipLaunchKernelGGL((pq_gqa_kernel<T, true>), grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((pq_gqa_kernel<T, false>), grid, dim3(256), 0, stream, p);
  if (hipGetLastError() != hipSuccess) return SPATTEN_ERR_LAUNCH;
  if (a->flags & SPATTEN_PQ_MSB_PASS_ONLY) return SPATTEN_OK;
  const PqQintExtra qx{qa->q_int, qa->qi_sb, qa->qi_sh, qa->q_scale, p.qmax};
  return pq_qint_refetch(a, pd, qx, stream);
}

}  // namespace spatten

using namespace spatten;

extern "C" int spatten_pq_qint_gqa_supported(int dtype, int heads, int kv_heads, int head_dim, int key_msb_bits, int value_bits,
                                             int query_bits) {
  if (dtype != SPATTEN_BF16 && dtype != SPATTEN_F16) return 0;
  if (heads <= 0 || kv_heads <= 0 || heads % kv_heads != 0) return 0;
  const int g = heads / kv_heads;
  if (g < 2 || g > 32) return 0;
  if (head_dim != 128 || key_msb_bits != 8 || value_bits != 8) return 0;
  return query_bits >= 4 && query_bits <= 8;
}

extern "C" int spatten_attn_decode_pq_qint_gqa(const spatten_pq_qint_args_t* qa, void* stream) {
  if (!qa || qa->struct_size != sizeof(spatten_pq_qint_args_t)) return SPATTEN_ERR_INVALID;
  if (!qa->q_int || !qa->q_scale || qa->query_bits < 4 || qa->query_bits > 8) return SPATTEN_ERR_INVALID;
  const spatten_pq_decode_args_t* a = &qa->step;
  PlanesDev pd;
  const int rc = pq_validate(a, pd);
  if (rc != SPATTEN_OK) return rc;
  if (a->step_state_sb != 0) return SPATTEN_ERR_UNSUPPORTED;     // the grouped MSB pass reads the one shared state
  // (the exported query leaves as two 8-byte stores per lane and piece; the query rows are read 16 bytes at a time)
  if (((uintptr_t)qa->q_int | (uintptr_t)qa->qi_sb | (uintptr_t)qa->qi_sh) & 7u) return SPATTEN_ERR_INVALID;
  if (a->k_new != nullptr || a->head_ids != nullptr || a->head_abs_acc != nullptr) return SPATTEN_ERR_UNSUPPORTED;
  if (!spatten_pq_qint_gqa_supported(a->dtype, a->heads, a->kv_heads, a->head_dim, a->planes->key_msb_bits, a->planes->value_bits,
                                     qa->query_bits))
    return SPATTEN_ERR_UNSUPPORTED;
  if ((int64_t)a->kv_len * 128 >= 0x7FFFFFFFll) return SPATTEN_ERR_UNSUPPORTED;          // 32-bit byte offsets inside a plane
  if (!pd.lg) return SPATTEN_ERR_INVALID;
  if (a->dtype == SPATTEN_BF16) return run_pq_gqa<bf16_t>(qa, pd, (hipStream_t)stream);
  return run_pq_gqa<f16_t>(qa, pd, (hipStream_t)stream);
}
