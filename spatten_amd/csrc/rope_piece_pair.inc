// rope_piece_pair.inc — the rotated shadow of a moved row's 16-byte piece PAIR, included INTO the row movers (prune.hip:
// kv_compact_kernel; prune_ragged.hip: prune_ragged_compact_kernel).  A textual fragment for the reason select_reg_body.inc gives:
// the statements compile exactly as they did inside kv_compact_kernel.
//
// Expects in scope: T; u32x4 lo_v / hi_v (elements [e0, e0 + E) of the row and the same elements of its second half), cs / sn (the
// rotary half-table pieces of the row's NEW position); char* rbase, int64_t doff, int half_bytes (where the shadow's pair goes).
// modify_llama.py:21-28 with the reference's roundings.
    constexpr int E = 16 / sizeof(T);              // elements per 16-byte piece (8, or 4 for fp32)
    const T* xl = reinterpret_cast<const T*>(&lo_v);
    const T* xh = reinterpret_cast<const T*>(&hi_v);
    const T* cc = reinterpret_cast<const T*>(&cs);
    const T* ss = reinterpret_cast<const T*>(&sn);
    u32x4 olo, ohi;
    T* yl = reinterpret_cast<T*>(&olo);
    T* yh = reinterpret_cast<T*>(&ohi);
    {
#pragma clang fp contract(off)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float a = DT<T>::to_f32(xl[e]), bb = DT<T>::to_f32(xh[e]);
        const float c = DT<T>::to_f32(cc[e]), s_ = DT<T>::to_f32(ss[e]);
        yl[e] = DT<T>::from_f32(DT<T>::round(a * c) + DT<T>::round(-bb * s_));
        yh[e] = DT<T>::from_f32(DT<T>::round(bb * c) + DT<T>::round(a * s_));
      }
    }
    __builtin_nontemporal_store(olo, reinterpret_cast<u32x4*>(rbase + doff));
    __builtin_nontemporal_store(ohi, reinterpret_cast<u32x4*>(rbase + doff + half_bytes));
