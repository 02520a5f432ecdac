// select_reg_body.inc — the body of the register window top-k, included INTO a kernel (prune.hip: topk_select_reg_kernel;
// prune_ragged.hip: prune_ragged_select_kernel).  A textual fragment and not a function on purpose: a kernel that hands its parameter
// block to a function takes a private copy of it and loads every field at entry, which changes the instruction stream of the
// existing select kernels; included, the statements compile exactly as they did inside topk_select_reg_kernel.
//
// Expects in scope: the template parameters T, NT, VPT; SEL_WINDOW — statements that declare `const T* row` (the window's first
// score, contiguous), `int32_t* out` (its k results) and `const int W` (0 < k <= W <= NT * VPT), all workgroup-uniform; and a block
// `p` with int members `lo` (added to every kept position) and `k`.  Result: out[0..k) = lo + the kept positions, ascending; ties at
// the k-th value go to the lowest index; a window that fills only part of the registers skips the all-padding ones.
  constexpr int NW = NT / kWave;
  constexpr int NE = VPT * NW;                 // (slab, wave) cells of 64 consecutive scores, in window order
  constexpr int EPL = (NE + kWave - 1) / kWave;
  __shared__ unsigned s_tot[3][2];
  __shared__ unsigned s_cell[NE + 1];
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  SEL_WINDOW
  constexpr int kBits = sizeof(T) == 4 ? 32 : (DT<T>::kId == SPATTEN_BF16 ? 16 : 24);
  constexpr unsigned kKeyMask = kBits == 32 ? 0xFFFFFFFFu : (kBits == 24 ? 0xFFFFFF00u : 0xFFFF0000u);
  const unsigned k = (unsigned)p.k;

  // score j * NT + tid in register j: every load instruction of a wave reads 64 consecutive scores (r02: consecutive
  // scores per THREAD cost 7 us of address-divergent 2-byte loads at 16384 scores)
  unsigned key[VPT];
  {
    float f[VPT];                          // unconditional (clamped) loads, all VPT in flight at once: left to itself
#pragma unroll                             // the compiler sinks each load into its `i < W` branch, one round trip each
    for (int j = 0; j < VPT; ++j) f[j] = DT<T>::to_f32(row[min(j * NT + tid, W - 1)]);
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      asm volatile("" : "+v"(f[j]));
      key[j] = j * NT + tid < W ? (ordered_key(f[j]) & kKeyMask) : 0u;   // 0: below every real key
    }
  }
  const int jmax = (W + NT - 1) / NT;    // registers j >= jmax are padding in every thread: skipped below
  if (tid < 6) (&s_tot[0][0])[tid] = 0u;
  __syncthreads();

  unsigned t = 0;
  int pass = 0;
#pragma unroll 1
  for (int s = 30; s >= 32 - kBits; s -= 2, ++pass) {
    const int slot = pass % 3;
    unsigned acc = 0;                  // four byte counters: how many of my keys fall in class 0..3
    if (jmax == VPT) {
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const unsigned x = __builtin_elementwise_sub_sat(key[j], t);
        const unsigned d = min(x >> s, 3u);
        acc += 1u << (8u * d);
      }
    } else {                           // a window that fills only part of the registers: the all-padding ones are skipped
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        if (j >= jmax) break;
        const unsigned x = __builtin_elementwise_sub_sat(key[j], t);
        const unsigned d = min(x >> s, 3u);
        acc += 1u << (8u * d);
      }
    }
    const unsigned f3 = acc >> 24, f2 = (acc >> 16) & 255u, f1 = (acc >> 8) & 255u;
    const unsigned ge3 = f3, ge2 = f3 + f2, ge1 = ge2 + f1;
    const unsigned a = wave_sum_u32(ge1 | (ge2 << 16)), b3 = wave_sum_u32(ge3);
    if (lane == 0) { atomicAdd(&s_tot[slot][0], a); atomicAdd(&s_tot[slot][1], b3); }
    if (tid < 2) s_tot[(pass + 1) % 3][tid] = 0u;     // last read two barriers ago
    __syncthreads();
    const unsigned t0 = s_tot[slot][0], n3 = s_tot[slot][1], n1 = t0 & 0xFFFFu, n2 = t0 >> 16;
    t |= (n3 >= k ? 3u : (n2 >= k ? 2u : (n1 >= k ? 1u : 0u))) << s;
  }
  // t = key of the k-th largest.  Order-preserving compaction: packed (greater, equal) counts per cell, one scan over
  // the cells, lane offsets from the ballots.
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const unsigned long long m_gt = __ballot(key[j] > t);
    const unsigned long long m_eq = __ballot(key[j] == t && j * NT + tid < W);
    if (lane == 0) s_cell[j * NW + wave] = ((unsigned)__popcll(m_gt) << 16) | (unsigned)__popcll(m_eq);   // <= 32768 each
  }
  __syncthreads();
  if (wave == 0) {
    unsigned c[EPL], tot = 0;
#pragma unroll
    for (int u = 0; u < EPL; ++u) { c[u] = (lane * EPL + u < NE) ? s_cell[lane * EPL + u] : 0u; tot += c[u]; }
    unsigned inc = tot;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const unsigned v = __shfl_up(inc, off, kWave);
      if (lane >= off) inc += v;
    }
    unsigned ex = inc - tot;
#pragma unroll
    for (int u = 0; u < EPL; ++u) { if (lane * EPL + u < NE) s_cell[lane * EPL + u] = ex; ex += c[u]; }
    if (lane == kWave - 1) s_cell[NE] = inc;
  }
  __syncthreads();
  const unsigned need_eq = k - (s_cell[NE] >> 16);      // >= 1: that many keys equal to t are kept, lowest index first
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int i = j * NT + tid;
    const bool gt = key[j] > t, eq = key[j] == t && i < W;
    const unsigned long long m_gt = __ballot(gt), m_eq = __ballot(eq);
    const unsigned ex = s_cell[j * NW + wave];
    const unsigned g = (ex >> 16) + __builtin_amdgcn_mbcnt_hi((unsigned)(m_gt >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m_gt, 0u));
    const unsigned e = (ex & 0xFFFFu) + __builtin_amdgcn_mbcnt_hi((unsigned)(m_eq >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m_eq, 0u));
    if (gt) out[g + (e < need_eq ? e : need_eq)] = p.lo + i;
    else if (eq && e < need_eq) out[g + e] = p.lo + i;
  }
