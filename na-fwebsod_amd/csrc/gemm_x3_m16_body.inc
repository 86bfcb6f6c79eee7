// Body of gemm_x3_m16_kernel / gemm_x3_m16p_kernel (gemm_x3.hip): included once per kernel with
// NAWS_M16_PIPE = false (the two-phase K loop) or true (the software-pipelined one), so that tile
// mapping, DMA pieces and epilogues exist once and the two-phase kernels keep their code.
  static_assert(KS % 2 == 0, "a 16x16x32 MFMA spans two 16-deep slabs");
  static_assert(!SGD || (NPL == 1 && !F16), "the update epilogue: the bf16 plan's one-plane form");
  static_assert(!F16 || NPL <= 2, "f16 operands have one or two planes");
  typedef typename OperandVec<F16>::type vec_t;
  constexpr int NT = 64 * WM * WN;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TI = WTM / 16, TJ = WTN / 16;
  constexpr int IH = TI >= 8 ? 2 : 1, TIH = TI / IH;        // A fragments are read in row halves
  constexpr int A_PLANE = BM * 32, B_PLANE = BN * 32;
  constexpr int NQ = NPL * KS;
  constexpr int STAGE = NQ * (A_PLANE + B_PLANE);
  constexpr int PIECE_ROWS = NT / 2;
  // DMA pieces (1 KB = 32 rows of one plane-slab).  Tiles whose sides are multiples of the
  // workgroup's PIECE_ROWS use the round form (wave w takes rows p * PIECE_ROWS + 32 w of every
  // plane-slab); other tiles (256 x 128 on 8 waves) deal the flat piece list round-robin:
  // piece q = wid + NW k, the first NQ BM / 32 of them A pieces.
  constexpr bool ROUND = BM % PIECE_ROWS == 0 && BN % PIECE_ROWS == 0;
  constexpr int NW = WM * WN;
  constexpr int PA = ROUND ? BM / PIECE_ROWS : 1, PB = ROUND ? BN / PIECE_ROWS : 1;
  constexpr int NPA = NQ * BM / 32, NPB = NQ * BN / 32;      // pieces per step
  constexpr int G = ROUND ? NQ * (PA + PB) : (NPA + NPB) / NW;
  static_assert(ROUND || (NPA % NW == 0 && NPB % NW == 0), "tile vs workgroup");
  static_assert((STAGES - 2) * G <= 63, "vmcnt range");
  extern __shared__ __attribute__((aligned(16))) unsigned char smx[];

  // Workgroups go to the 8 XCDs round-robin by launch index.  The (batch item, tile) space is cut
  // into 8 contiguous ranges, one per XCD: within a batch item an XCD's L2 sees neighbouring
  // tiles, and a batched launch (the 16 Winograd frequencies) keeps whole batch items on one XCD,
  // so every operand is fetched into ONE L2 instead of all eight (PMC: 301 MB fetched per launch
  // for 95 MB of operands when each frequency's tiles were spread over the XCDs)
  const int ntiles = g.tiles_m * g.tiles_n;
  int lid = blockIdx.x;
  {
    const int total = ntiles * g.batch;
    const int q = total >> 3, rem = total & 7, xcd = lid & 7, within = lid >> 3;
    lid = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + within;
  }
  const long long bz = lid / ntiles;
  lid -= (int)bz * ntiles;
  constexpr int GM = 8;
  const int per_group = GM * g.tiles_n;
  const int grp = lid / per_group;
  const int first_m = grp * GM;
  const int gsz = min(g.tiles_m - first_m, GM);
  const int tm = first_m + (lid % per_group) % gsz;
  const int tn = (lid % per_group) / gsz;
  const int m0 = tm * BM, n0 = tn * BN;

  const unsigned short* A = g.A + bz * g.sA;
  const unsigned short* B = g.B + bz * g.sB;
  float* C = g.C + bz * g.sC;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int l15 = lane & 15, kg = lane >> 4;

  const int lrow = tid >> 1;
  const int kslot = (tid & 1) * 8;
  const unsigned short* srcA[PA];
  const unsigned short* srcB[PB];
#pragma unroll
  for (int p = 0; p < PA; ++p)
    srcA[p] = A + (long long)min(m0 + p * PIECE_ROWS + lrow, g.M - 1) * 16 + kslot;
#pragma unroll
  for (int p = 0; p < PB; ++p)
    srcB[p] = B + (long long)min(n0 + p * PIECE_ROWS + lrow, g.N - 1) * 16 + kslot;

  // flat form: this wave's pieces
  constexpr int GF = ROUND ? 1 : G;
  const unsigned short* fsrc[GF];
  int fdst[GF];
  if constexpr (!ROUND) {
    const int r32 = lane >> 1;
#pragma unroll
    for (int kq = 0; kq < GF; ++kq) {
      const int q = wid + NW * kq;
      if (kq < NPA / NW) {
        const int pq = q / (BM / 32), rg = q % (BM / 32);
        fsrc[kq] = A + (long long)(pq / KS) * g.planeA + (long long)(pq % KS) * g.slabA +
                   (long long)min(m0 + rg * 32 + r32, g.M - 1) * 16 + (lane & 1) * 8;
        fdst[kq] = pq * A_PLANE + rg * 1024;
      } else {
        const int q2 = q - NPA;
        const int pq = q2 / (BN / 32), rg = q2 % (BN / 32);
        fsrc[kq] = B + (long long)(pq / KS) * g.planeB + (long long)(pq % KS) * g.slabB +
                   (long long)min(n0 + rg * 32 + r32, g.N - 1) * 16 + (lane & 1) * 8;
        fdst[kq] = NQ * A_PLANE + pq * B_PLANE + rg * 1024;
      }
    }
  }
  auto issue = [&](int t, int st) {
    if constexpr (!ROUND) {
      unsigned char* base = smx + st * STAGE;
#pragma unroll
      for (int kq = 0; kq < GF; ++kq) {
        const long long adv = (long long)(t * KS) * (kq < NPA / NW ? g.slabA : g.slabB);
        __builtin_amdgcn_global_load_lds(NAWS_GLB_PTR(fsrc[kq] + adv), NAWS_LDS_PTR(base + fdst[kq]),
                                         16, 0, 0);
      }
      return;
    }
    unsigned char* base = smx + st * STAGE + wid * 1024;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int pl = q / KS, ks = q % KS;
      const long long ka = (long long)(t * KS + ks) * g.slabA, kb = (long long)(t * KS + ks) * g.slabB;
#pragma unroll
      for (int p = 0; p < PA; ++p)
        __builtin_amdgcn_global_load_lds(NAWS_GLB_PTR(srcA[p] + pl * g.planeA + ka),
                                         NAWS_LDS_PTR(base + q * A_PLANE + p * (NT * 16)), 16, 0, 0);
#pragma unroll
      for (int p = 0; p < PB; ++p)
        __builtin_amdgcn_global_load_lds(NAWS_GLB_PTR(srcB[p] + pl * g.planeB + kb),
                                         NAWS_LDS_PTR(base + NQ * A_PLANE + q * B_PLANE + p * (NT * 16)),
                                         16, 0, 0);
    }
  };

  f32x4 acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

  // lane -> (row l15, slab kg >> 1 of the pair, k-half kg & 1)
  const int rd_a = (wm * WTM + l15) * 32 + (kg & 1) * 16 + (kg >> 1) * A_PLANE;
  const int rd_b = NQ * A_PLANE + (wn * WTN + l15) * 32 + (kg & 1) * 16 + (kg >> 1) * B_PLANE;

  const int T = g.K / (16 * KS);
  if constexpr (NAWS_M16_PIPE) {
    // ---- the software-pipelined loop (DESIGN 3b) ------------------------------------------------
    // A step = SP sub-phases of two column fragments (2 x TI accumulators, 3 terms each).  The A
    // fragments of a step stay resident (a0[step & 1], a1); the B fragments stream in two-fragment sets
    // b[0] / b[1], the set of sub-phase s + 1 read BEFORE the MFMAs of sub-phase s.  The step's one
    // vmcnt wait and barrier sit before the LAST sub-phase: by then this wave has read all of
    // stage t (the lgkmcnt(0) in front of the barrier retires its last B set), so behind the
    // barrier stage t's slot is free for the DMA of step t + 2 and stage t + 1 - whose DMA every
    // wave has waited for - is readable: step t + 1's hi A fragments and first B set are read under
    // the last sub-phase's MFMAs.  Barriers: one in the prologue and one per step but the last;
    // every condition is a function of T alone.  Per accumulator the products arrive in the
    // parent loop's order ((0,0), (0,1), (1,0) per step): results are bit-identical.
    static_assert(F16 && NPL == 2 && KS == 2 && STAGES == 2 && IH == 1 && TJ % 4 == 0 && ROUND && !SGD,
                  "the pipelined loop: fp16x2, 32-deep steps, two stages");
    constexpr int SP = TJ / 2;
    // Registers: 4 TI TJ accumulators + a0 double-buffered (2 x 4 TI) + a1 (4 TI) + two B sets
    // (2 x 16) = 128 + 80 at this tile.  The lo A plane a1 is needed by a sub-phase's LAST term
    // only, so step t + 1's copy is read at the head of ITS sub-phase 0 over step t's - one set.
    // The DMA's global addresses are written as uniform base + 32-bit lane offset: only the two
    // offsets live across the loop instead of a 64-bit pointer per piece (the address pair of a
    // piece is formed at its issue, v_lshl_add_u64).  srcA / srcB / fsrc / issue above are the
    // two-phase loop's and dead in this instantiation.
    vec_t a0[2][TI], a1[TI], b[2][NPL][2];
    unsigned offA[PA], offB[PB];              // bytes from a plane-slab's first row
#pragma unroll
    for (int p = 0; p < PA; ++p)
      offA[p] = (unsigned)(min(m0 + p * PIECE_ROWS + lrow, g.M - 1) * 16 + kslot) * 2u;
#pragma unroll
    for (int p = 0; p < PB; ++p)
      offB[p] = (unsigned)(min(n0 + p * PIECE_ROWS + lrow, g.N - 1) * 16 + kslot) * 2u;
    auto issue_p = [&](int t, int st) {        // the pieces of issue(), addressed as above
      unsigned char* base = smx + st * STAGE + wid * 1024;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int pl = q / KS, ks = q % KS;
        const unsigned char* ua =
            reinterpret_cast<const unsigned char*>(A + pl * g.planeA + (long long)(t * KS + ks) * g.slabA);
        const unsigned char* ub =
            reinterpret_cast<const unsigned char*>(B + pl * g.planeB + (long long)(t * KS + ks) * g.slabB);
#pragma unroll
        for (int p = 0; p < PA; ++p)
          __builtin_amdgcn_global_load_lds(NAWS_GLB_PTR(ua + offA[p]),
                                           NAWS_LDS_PTR(base + q * A_PLANE + p * (NT * 16)), 16, 0, 0);
#pragma unroll
        for (int p = 0; p < PB; ++p)
          __builtin_amdgcn_global_load_lds(NAWS_GLB_PTR(ub + offB[p]),
                                           NAWS_LDS_PTR(base + NQ * A_PLANE + q * B_PLANE + p * (NT * 16)),
                                           16, 0, 0);
      }
    };
    // The fragment reads are inline asm: behind an LDS-DMA hipcc drains every LDS wait to
    // lgkmcnt(0) (it counts the DMA as an out-of-order LDS access), which would put each set's
    // latency back in front of its MFMAs.  The compiler therefore sees no LDS read in this loop and
    // the waits are written by hand, with the loop, in gemm_h2_pipe_loop.inc.
    const unsigned lds_a[2] = {(unsigned)(size_t)NAWS_LDS_PTR(smx + rd_a),
                               (unsigned)(size_t)NAWS_LDS_PTR(smx + STAGE + rd_a)};
    const unsigned lds_b[2] = {(unsigned)(size_t)NAWS_LDS_PTR(smx + rd_b),
                               (unsigned)(size_t)NAWS_LDS_PTR(smx + STAGE + rd_b)};
    static_assert(KS * A_PLANE + TI * 512 < 65536 && KS * B_PLANE + TJ * 512 < 65536, "ds offset field");
#define NAWS_M16P_LDS(DST, ADDR, OFF) \
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(DST) : "v"(ADDR), "n"(OFF) : "memory");
#define NAWS_PIPE_READ_A(DST, PL, STG)           \
  _Pragma("unroll") for (int i = 0; i < TI; ++i) \
      NAWS_M16P_LDS(DST[i], lds_a[STG], (PL) * KS * A_PLANE + i * 512)
#define NAWS_PIPE_READ_B(SET, STG, SPH)                                                         \
  _Pragma("unroll") for (int pl = 0; pl < NPL; ++pl) _Pragma("unroll") for (int jj = 0; jj < 2; ++jj) \
      NAWS_M16P_LDS(b[SET][pl][jj], lds_b[STG], pl * KS * B_PLANE + ((SPH) * 2 + jj) * 512)
#define NAWS_PIPE_NB 4                       /* 2 planes x 2 column fragments */
#define NAWS_PIPE_PIECES G
#define NAWS_PIPE_MFMA(B, A, C) mfma32(B, A, C)
#include "gemm_h2_pipe_loop.inc"
#undef NAWS_PIPE_MFMA
#undef NAWS_PIPE_PIECES
#undef NAWS_PIPE_NB
#undef NAWS_M16P_LDS
#undef NAWS_PIPE_READ_B
#undef NAWS_PIPE_READ_A
  } else {
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < T) issue(s, s);
  int st_cur = 0, st_fill = STAGES - 1;
  for (int t = 0; t < T; ++t) {
    if (t + STAGES - 2 < T) wait_vmcnt<(STAGES - 2) * G>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (t + STAGES - 1 < T) issue(t + STAGES - 1, st_fill);
    const unsigned char* st = smx + st_cur * STAGE;
#pragma unroll
    for (int kk = 0; kk < KS / 2; ++kk) {
      vec_t b[NPL][TJ];
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
          b[pl][j] = *reinterpret_cast<const vec_t*>(st + rd_b + (pl * KS + 2 * kk) * B_PLANE + j * 512);
#pragma unroll
      for (int ih = 0; ih < IH; ++ih) {
        vec_t a[NPL][TIH];
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
          for (int i = 0; i < TIH; ++i)
            a[pl][i] = *reinterpret_cast<const vec_t*>(st + rd_a + (pl * KS + 2 * kk) * A_PLANE +
                                                       (ih * TIH + i) * 512);
#define NAWS_M16_TERM(P, Q)                                                                      \
  _Pragma("unroll") for (int i = 0; i < TIH; ++i) _Pragma("unroll") for (int j = 0; j < TJ; ++j) \
      acc[ih * TIH + i][j] = mfma32(b[Q][j], a[P][i], acc[ih * TIH + i][j]);
        NAWS_M16_TERM(0, 0)
        if constexpr (NPL >= 2) {
          NAWS_M16_TERM(0, 1)
          NAWS_M16_TERM(1, 0)
        }
        if constexpr (NPL == 3) {                     // the exact 3 x bf16 split: six terms
          NAWS_M16_TERM(1, 1)
          NAWS_M16_TERM(0, 2)
          NAWS_M16_TERM(2, 0)
        }
#undef NAWS_M16_TERM
      }
    }
    st_cur = (st_cur + 1 == STAGES) ? 0 : st_cur + 1;
    st_fill = (st_fill + 1 == STAGES) ? 0 : st_fill + 1;
  }
  }

  // The MFMAs above ran with the operands swapped (B fragment first): an accumulator block is the
  // TRANSPOSED 16x16 block of C, i.e. lane (l15, kg) holds row l15, columns kg * 4 + e - four
  // consecutive columns of one row (same products, same k order: bit-identical to the un-swapped
  // form, which holds four rows of one column).  The epilogue therefore moves 16 bytes per lane
  // (C, aux, bias, column factors) wherever the layout allows (g.vec4), 4x fewer memory
  // instructions than the 4-byte form: the aux-reading fc7 dgrad 0.72 -> see DESIGN 0a.
  if constexpr (SGD) {
    // ---- the update in place of the store (one process, no gradient exchange in between;
    // gemm_btr.hip's SGD form for the bf16 plan): the product is the gradient element, then
    // acm_sgd_planes_kernel<2>'s element work - sgd_elem, momentum and parameter written back,
    // the updated weight rounded to the bf16 operand plane (a lane's four columns = 8 bytes; a
    // fragment's 16 rows x 32 bytes = one contiguous 512-byte run of the K-slab).  All of a row
    // group's loads are issued before its arithmetic and stores.
    const float LR = g.lr[0] * g.lr_mult;
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      const int row = m0 + wm * WTM + i * 16 + l15;
      const bool row_on = row < g.M;
      const int rr = row_on ? row : g.M - 1;
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
        if (!row_on || col >= g.N) continue;          // N % 16 == 0: four columns in or out together
        const f32x4 v = acc[i][j];
        const long long o = (long long)row * g.ldp + col;
        f32x4 p = pw[j], m = pm[j];
        unsigned short q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float me = m[e], pe = p[e];
          sgd_elem(v[e], me, pe, g.gscale, g.wd, LR, g.momentum, g.nesterov);
          m[e] = me; p[e] = pe;
          const __bf16 h = (__bf16)pe;
          q[e] = *reinterpret_cast<const unsigned short*>(&h);
        }
        *reinterpret_cast<f32x4*>(g.mom + o) = m;
        *reinterpret_cast<f32x4*>(g.param + o) = p;
        const long long po = ((long long)(col >> 4) * g.prows + row) * 16 + (col & 15);
        *reinterpret_cast<uint2*>(g.P + po) =
            make_uint2(q[0] | ((unsigned)q[1] << 16), q[2] | ((unsigned)q[3] << 16));
      }
    }
    return;
  }
  const float* bias = g.bias ? g.bias + bz * g.sBias : nullptr;
  const float* aux = g.aux ? g.aux + bz * g.sC : nullptr;
  const int epi = g.epilogue;
  const bool has_bias = bias && epi >= NAWS_EPI_BIAS && epi <= NAWS_EPI_BIAS_RELU_DROP;
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const int row = m0 + wm * WTM + i * 16 + l15;
    float rsv = 1.f;
    if constexpr (F16) rsv = (g.rs + bz * g.sRs)[min(row, g.M - 1)];
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int col = n0 + wn * WTN + j * 16 + kg * 4;
      f32x4 v = acc[i][j];
      if (row < g.M && col < g.N) {
        const bool full = g.vec4 && col + 3 < g.N;
        f32x4 bv = {0.f, 0.f, 0.f, 0.f}, cs = {1.f, 1.f, 1.f, 1.f}, ax = {0.f, 0.f, 0.f, 0.f},
              old = {0.f, 0.f, 0.f, 0.f};
        float* cp = C + (long long)row * g.ldc + col;
        const float* ap = aux ? aux + (long long)row * g.ldaux + col : nullptr;
        if (full) {
          if (has_bias) bv = *reinterpret_cast<const f32x4*>(bias + col);
          if constexpr (F16) cs = *reinterpret_cast<const f32x4*>(g.cs + bz * g.sCs + col);
          if (epi == NAWS_EPI_GATE_POS) ax = *reinterpret_cast<const f32x4*>(ap);
          if (g.accumulate) old = *reinterpret_cast<const f32x4*>(cp);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (col + e >= g.N) continue;
            if (has_bias) bv[e] = bias[col + e];
            if constexpr (F16) cs[e] = g.cs[bz * g.sCs + col + e];
            if (epi == NAWS_EPI_GATE_POS) ax[e] = ap[e];
            if (g.accumulate) old[e] = cp[e];
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float t = v[e];
          if constexpr (F16) t = t * rsv * cs[e];          // powers of two: exact, in this order
          t += bv[e];
          if (epi == NAWS_EPI_BIAS_RELU || epi == NAWS_EPI_BIAS_RELU_DROP) t = fmaxf(t, 0.f);
          if (epi == NAWS_EPI_BIAS_RELU_DROP) {
            const unsigned long long dld = g.drop_ld ? g.drop_ld : g.N;
            const unsigned long long idx =
                (unsigned long long)bz * g.M * dld + (unsigned long long)row * dld + (g.drop_c0 + col + e);
            t = naws_keep(g.seed, idx, g.drop_thr) ? t * g.drop_scale : 0.f;
          } else if (epi == NAWS_EPI_GATE_POS) {
            t = (ax[e] > 0.f) ? t * g.alpha : 0.f;
          }
          if (g.accumulate) t += old[e];
          v[e] = t;
        }
        if (full) {
          *reinterpret_cast<f32x4*>(cp) = v;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (col + e < g.N) cp[e] = v[e];
        }
      }
      acc[i][j] = v;
    }
  }
  if (g.am.rowmax || g.am.colmax)
    naws_tile_amax_16t<TI, TJ>(acc, m0 + wm * WTM, n0 + wn * WTN, g.M, g.N, lane, g.am, bz);
