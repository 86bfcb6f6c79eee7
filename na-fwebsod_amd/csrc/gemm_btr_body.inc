// Body of gemm_h2_btr_kernel / gemm_h2_btrp_kernel (gemm_btr.hip): included once per kernel with
// NAWS_BTR_PIPE = false (the two-phase K loop) or true (the software-pipelined one), so that tile
// mapping, DMA pieces and epilogues exist once and the two-phase kernels keep their code.
  constexpr int NT = 64 * WM * WN, NW = WM * WN;
  constexpr int WTM = BM / WM, WTN = BN / WN, TI = WTM / 16, TJ = WTN / 16;
  constexpr int A_PLANE = BM * 32, B_PLANE = BN * 32;
  constexpr int STAGE = NQ * (A_PLANE + B_PLANE);
  static_assert(BM == NT / 2, "one DMA round = one (plane, slab) of the A tile");
  static_assert(BN / 16 == 2 * NW && WTN / 16 == NW, "two rounds of NW feature blocks per plane; a wave's columns = one round");
  extern __shared__ __attribute__((aligned(16))) unsigned char smx[];
  const int ntiles = g.tiles_m * g.tiles_n;
  int lid = blockIdx.x;
  {
    const int q = ntiles >> 3, rem = ntiles & 7, xcd = lid & 7, within = lid >> 3;
    lid = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + within;
  }
  constexpr int GM = 8;
  const int per_group = GM * g.tiles_n;
  const int grp = lid / per_group;
  const int first_m = grp * GM;
  const int gsz = min(g.tiles_m - first_m, GM);
  const int tm = first_m + (lid % per_group) % gsz;
  const int tn = (lid % per_group) / gsz;
  const int m0 = tm * BM, n0 = tn * BN;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int l15 = lane & 15, kg = lane >> 4;

  // A: thread -> (row tid >> 1, k-half tid & 1) of a 256-row plane-slab
  const unsigned short* srcA = g.A + (long long)min(m0 + (tid >> 1), g.M - 1) * 16 + (tid & 1) * 8;
  // B: a workgroup round = NW feature blocks x 1 KB; wave -> feature block, lane -> 16-B chunk c of
  // the block's LDS image = (slot c >> 1, feature half c & 1); slot -> proposal by the bit swap
  const int slot = lane >> 1;
  const int prop = (slot & 0x13) | ((slot & 4) << 1) | ((slot & 8) >> 1);
  const int nfb = g.N / 16;
  const unsigned short* srcX[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    srcX[ks] = g.X + (long long)min(n0 / 16 + ks * NW + wid, nfb - 1) * g.slabX + (lane & 1) * 8;

  auto issue = [&](int t, int st) {
    unsigned char* base = smx + st * STAGE + wid * 1024;
    const long long xr = (long long)min(t * 32 + prop, g.xrows - 1) * 16;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int pl = q / KS, ks = q % KS;
      __builtin_amdgcn_global_load_lds(
          NAWS_GLB_PTR(srcA + pl * g.planeA + (long long)(t * KS + ks) * g.slabA),
          NAWS_LDS_PTR(base + q * A_PLANE), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(NAWS_GLB_PTR(srcX[ks] + pl * g.planeX + xr),
                                       NAWS_LDS_PTR(base + NQ * A_PLANE + q * B_PLANE), 16, 0, 0);
    }
  };

  f32x4 acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

  const int rd_a = (wm * WTM + l15) * 32 + (kg & 1) * 16 + (kg >> 1) * A_PLANE;
  // transposed read: lane 4q + p of a 16-lane group addresses slot row q, features 4p .. 4p + 3;
  // k-group kg, first / second half of its 8 proposals -> slot (kg >> 1) * 16 + hh * 8 + (kg & 1) * 4 + q
  const int tq = (lane & 15) >> 2, tp = lane & 3;
  const int rd_b = NQ * A_PLANE + wn * B_PLANE + ((kg >> 1) * 16 + (kg & 1) * 4 + tq) * 32 + tp * 8;

  const int T = g.K / 32;
  if constexpr (NAWS_BTR_PIPE) {
    // ---- the software-pipelined loop: the schedule of gemm_x3_m16_body.inc (DESIGN 3b) ----------
    // A step = SP sub-phases of two feature blocks (2 x TI accumulators, 3 terms each).  a0 (the hi
    // A plane) is double-buffered over steps, a1 (lo, needed by a sub-phase's last term only) is
    // read at the head of its step's sub-phase 0, the B fragments stream in two sets, set s + 1
    // read before the MFMAs of sub-phase s.  The step's vmcnt wait and barrier stand before the last
    // sub-phase: this wave has then read all of stage t (lgkmcnt(0)), so behind the barrier the DMA
    // of step t + 2 may refill it and stage t + 1 is readable.  One barrier in the prologue, one
    // per step but the last; every condition is a function of T.  Per accumulator the products
    // arrive in the two-phase loop's order: bit-identical.
    // EVERY LDS read of this loop is inline asm (the A reads too: behind the LDS-DMA hipcc would
    // drain its own reads with lgkmcnt(0)); the loop and its hand-counted waits are the shared
    // gemm_h2_pipe_loop.inc.  A B set is 8 reads here (2 planes x 2 blocks x 2 halves).
    static_assert(TI == 4 && TJ % 4 == 0, "the pipelined loop: waves of 64 x 128");
    // issue()'s pieces, their global addresses written as uniform base + 32-bit lane offset: only
    // the offsets live across the loop, the per-piece bases advance in scalar registers (the 64-bit
    // address pair of a piece is formed at its issue, v_lshl_add_u64).  srcA / srcX / issue above
    // are the two-phase loop's and dead in this instantiation.
    const unsigned offA = (unsigned)(min(m0 + (tid >> 1), g.M - 1) * 16 + (tid & 1) * 8) * 2u;
    const unsigned short* baseX[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      baseX[ks] = g.X + (long long)min(n0 / 16 + ks * NW + wid, nfb - 1) * g.slabX;
    auto issue_p = [&](int t, int st) {
      unsigned char* base = smx + st * STAGE + wid * 1024;
      const unsigned offX = (unsigned)(min(t * 32 + prop, g.xrows - 1) * 16 + (lane & 1) * 8) * 2u;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int pl = q / KS, ks = q % KS;
        const unsigned char* ua = reinterpret_cast<const unsigned char*>(
            g.A + pl * g.planeA + (long long)(t * KS + ks) * g.slabA);
        const unsigned char* ux = reinterpret_cast<const unsigned char*>(baseX[ks] + pl * g.planeX);
        __builtin_amdgcn_global_load_lds(NAWS_GLB_PTR(ua + offA), NAWS_LDS_PTR(base + q * A_PLANE), 16, 0, 0);
        __builtin_amdgcn_global_load_lds(NAWS_GLB_PTR(ux + offX),
                                         NAWS_LDS_PTR(base + NQ * A_PLANE + q * B_PLANE), 16, 0, 0);
      }
    };
    constexpr int SP = TJ / 2;
    typedef short i16x8 __attribute__((ext_vector_type(8)));
    f16x8 a0[2][TI], a1[TI];
    f16x8 b[2][NPL][2];
    const unsigned lds_a[2] = {(unsigned)(size_t)NAWS_LDS_PTR(smx + rd_a),
                               (unsigned)(size_t)NAWS_LDS_PTR(smx + STAGE + rd_a)};
    const unsigned lds_b[2] = {(unsigned)(size_t)NAWS_LDS_PTR(smx + rd_b),
                               (unsigned)(size_t)NAWS_LDS_PTR(smx + STAGE + rd_b)};
    static_assert(KS * A_PLANE + TI * 512 < 65536 && KS * B_PLANE + TJ * 1024 < 65536, "ds offset field");
#define NAWS_PIPE_READ_A(DST, PL, STG)                                                    \
  _Pragma("unroll") for (int i = 0; i < TI; ++i)                                          \
      asm volatile("ds_read_b128 %0, %1 offset:%2"                                        \
                   : "=v"(DST[i])                                                         \
                   : "v"(lds_a[STG]), "n"((PL) * (KS * A_PLANE) + i * 512)                \
                   : "memory");
#define NAWS_PIPE_READ_B(SET, STG, SPH)                                                   \
  _Pragma("unroll") for (int pl = 0; pl < NPL; ++pl) _Pragma("unroll") for (int jj = 0; jj < 2; ++jj) { \
    i16x4 lo, hi;                                                                         \
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"                                    \
                 : "=v"(lo)                                                               \
                 : "v"(lds_b[STG]), "n"(pl * (KS * B_PLANE) + ((SPH) * 2 + jj) * 1024)    \
                 : "memory");                                                             \
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"                                    \
                 : "=v"(hi)                                                               \
                 : "v"(lds_b[STG]), "n"(pl * (KS * B_PLANE) + ((SPH) * 2 + jj) * 1024 + 256) \
                 : "memory");                                                             \
    /* (register naming only, as in the two-phase loop: the halves ARE the fragment's registers) */ \
    const i16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);              \
    b[SET][pl][jj] = *reinterpret_cast<const f16x8*>(&v);                                 \
  }
#define NAWS_PIPE_NB 8                       /* 2 planes x 2 blocks x 2 halves */
#define NAWS_PIPE_PIECES (NQ * 2)
#define NAWS_PIPE_MFMA(B, A, C) __builtin_amdgcn_mfma_f32_16x16x32_f16(B, A, C, 0, 0, 0)
#include "gemm_h2_pipe_loop.inc"
#undef NAWS_PIPE_MFMA
#undef NAWS_PIPE_PIECES
#undef NAWS_PIPE_NB
#undef NAWS_PIPE_READ_B
#undef NAWS_PIPE_READ_A
  } else {
  issue(0, 0);
  int st_cur = 0;
  for (int t = 0; t < T; ++t) {
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (t + 1 < T) issue(t + 1, st_cur ^ 1);
    const unsigned char* st = smx + st_cur * STAGE;
    // (inline asm: behind the builtin form hipcc puts s_waitcnt vmcnt(0) - it cannot tell the
    // transposed read from the LDS-DMA's destination - which waits out the NEXT step's DMA in
    // every step; the fragments' own latency is retired by frag_fence below)
    f16x8 b[NPL][TJ];
    const unsigned bbase = (unsigned)(size_t)NAWS_LDS_PTR(st + rd_b);
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        const unsigned p = bbase + pl * (KS * B_PLANE) + j * 1024;
        i16x4 lo, hi;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(p));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:256" : "=v"(hi) : "v"(p));
        typedef short i16x8 __attribute__((ext_vector_type(8)));
        const i16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        b[pl][j] = *reinterpret_cast<const f16x8*>(&v);
      }
    frag_fence<TJ>(b[0], true);
    frag_fence<TJ>(b[1], false);
#pragma unroll
    for (int ih = 0; ih < 2; ++ih) {
      f16x8 a[NPL][TI / 2];
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
        for (int i = 0; i < TI / 2; ++i)
          a[pl][i] = *reinterpret_cast<const f16x8*>(st + rd_a + pl * (KS * A_PLANE) +
                                                     (ih * (TI / 2) + i) * 512);
#define NAWS_BTR_TERM(P, Q)                                                                       \
  _Pragma("unroll") for (int i = 0; i < TI / 2; ++i) _Pragma("unroll") for (int j = 0; j < TJ; ++j) \
      acc[ih * (TI / 2) + i][j] =                                                                 \
          __builtin_amdgcn_mfma_f32_16x16x32_f16(b[Q][j], a[P][i], acc[ih * (TI / 2) + i][j], 0, 0, 0);
      NAWS_BTR_TERM(0, 0)
      NAWS_BTR_TERM(0, 1)
      NAWS_BTR_TERM(1, 0)
#undef NAWS_BTR_TERM
    }
    st_cur ^= 1;
  }
  }

  // the MFMAs ran with the operands swapped (B fragment first): the accumulator block is C^T, so a
  // lane holds FOUR CONSECUTIVE COLUMNS of one row - row l15, columns kg * 4 + e - and the
  // epilogue moves 16 bytes per lane (the products and their k order are the same: bit-identical
  // to the un-swapped form, which holds four rows of one column and stores 4 bytes at a time)
  if constexpr (SGD) {
    // ---- the update in place of the store (one process, no gradient exchange between the two:
    // reference optimizer_wsl.py adds its all-reduce ops only for NUM_GPUS > 1).  g = the value
    // the plain epilogue would have stored; then exactly acm_sgd_planes_kernel's element work:
    // sgd_elem, the updated weight scaled by the row's bound-derived power of two and split into
    // the hi / lo f16 planes (a lane's four columns = 8 bytes per plane, a fragment's 16 rows x
    // 32 bytes = one contiguous 512-byte run of the K-slab), max|w| folded over the wave's
    // columns, one guarded atomic per (row, wave) and the overflow word.
    const float LR = g.lr[0] * g.lr_mult;
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      const int row = m0 + wm * WTM + i * 16 + l15;
      const bool row_on = row < g.M;
      const int rr = row_on ? row : g.M - 1;
      const float rsv = g.rs[rr];
      const unsigned bb = g.bound[rr];
      const unsigned b2 = ((bb >> 23) >= 1u && (bb >> 23) < 0xfeu) ? bb + (1u << 23) : bb;
      float sc, isc;
      naws_f16x2_scales(b2, sc, isc);
      if (row_on && n0 + wn * WTN == 0 && kg == 0) g.inv_scale[row] = isc;
      const long long prow = (long long)rr * 16;
      float mx = 0.f;
      bool bad = false;
      // all of the row group's parameter / momentum loads first (16 x 16 bytes in flight per
      // lane), then the arithmetic and the stores: fragment by fragment, every load waited
      // behind the previous fragment's stores (0.73 ms on the fc6 problem instead of 0.3)
      f32x4 pw[TJ], pm[TJ];
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        const int col = n0 + wn * WTN + j * 16 + kg * 4;
        const bool on = row_on && col < g.N;
        const long long o = (long long)rr * g.ldp + (on ? col : 0);
        pw[j] = *reinterpret_cast<const f32x4*>(g.param + o);
        if (!g.first) pm[j] = *reinterpret_cast<const f32x4*>(g.mom + o);
        else pm[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        const int col = n0 + wn * WTN + j * 16 + kg * 4;
        if (!row_on || col >= g.N) continue;
        f32x4 v = acc[i][j];
        if (g.cs) {
          const f32x4 c4 = *reinterpret_cast<const f32x4*>(g.cs + col);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] * rsv * c4[e];
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] * rsv;
        }
        const long long o = (long long)row * g.ldp + col;
        f32x4 p = pw[j], m = pm[j];
        unsigned short hq[4], lq[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float me = m[e], pe = p[e];
          sgd_elem(v[e], me, pe, g.gscale, g.wd, LR, g.momentum, g.nesterov);
          m[e] = me; p[e] = pe;
          mx = fmaxf(mx, fabsf(pe));
          bad = bad || (pe != pe);
          const float t = pe * sc;
          const _Float16 hi = (_Float16)t;
          float rem = t - (float)hi;
          if (!(fabsf(t) <= 65504.f)) rem = 0.f;         // NaN / overflow live in the hi plane only
          const _Float16 lo = (_Float16)rem;
          hq[e] = *reinterpret_cast<const unsigned short*>(&hi);
          lq[e] = *reinterpret_cast<const unsigned short*>(&lo);
        }
        *reinterpret_cast<f32x4*>(g.mom + o) = m;
        *reinterpret_cast<f32x4*>(g.param + o) = p;
        const long long po = (long long)(col >> 4) * g.prows * 16 + prow + (col & 15);
        *reinterpret_cast<uint2*>(g.P + po) =
            make_uint2(hq[0] | ((unsigned)hq[1] << 16), hq[2] | ((unsigned)hq[3] << 16));
        *reinterpret_cast<uint2*>(g.P + g.planeP + po) =
            make_uint2(lq[0] | ((unsigned)lq[1] << 16), lq[2] | ((unsigned)lq[3] << 16));
      }
      // (a NaN weight must reach the overflow test: fmaxf drops NaNs, so it travels as +inf)
      if (bad) mx = __uint_as_float(0x7f800000u);
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      if (kg == 0 && row_on) {
        const bool is_inf = __float_as_uint(mx) == 0x7f800000u;
        if (mx > 0.f && !is_inf) naws_atomic_max_bits(g.rowmax + row, mx);
        if (!(mx <= __uint_as_float(b2)) || is_inf) atomicMax(g.overflow, g.overflow_tag);
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const int row = m0 + wm * WTM + i * 16 + l15;
    if (row >= g.M) continue;
    const float rsv = g.rs[row];
    float* crow = g.C + (long long)row * g.ldc;
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int col = n0 + wn * WTN + j * 16 + kg * 4;
      if (col >= g.N) continue;                      // N % 16 == 0: the four columns are all in or out
      f32x4 v = acc[i][j];
      if (g.cs) {
        const f32x4 c4 = *reinterpret_cast<const f32x4*>(g.cs + col);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * rsv * c4[e];        // powers of two: exact
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * rsv;
      }
      *reinterpret_cast<f32x4*>(crow + col) = v;
    }
  }
