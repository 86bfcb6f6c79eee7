// The software-pipelined K loop shared by gemm_x3_m16p_kernel (gemm_x3_m16_body.inc) and
// gemm_h2_btrp_kernel (gemm_btr_body.inc): schedule, counted waits, barrier placement (DESIGN 3b).
// The including body defines, and undefines behind the include,
//   NAWS_PIPE_READ_A(DST, PL, STG)   TI inline-asm LDS reads of A plane PL of stage STG into DST[]
//   NAWS_PIPE_READ_B(SET, STG, SPH)  the NAWS_PIPE_NB inline-asm LDS reads of sub-phase SPH's two
//                                    column fragments (both planes) into b[SET]
//   NAWS_PIPE_NB                     LDS reads per B set (what the waits count)
//   NAWS_PIPE_MFMA(B, A, C)          one MFMA, operands swapped (B fragment first)
//   NAWS_PIPE_PIECES                 this wave's DMA pieces per step (the prologue's vmcnt)
// and has in scope: a0[2][TI], a1[TI], b[2][2][2], acc[TI][TJ], SP = TJ / 2, T, issue_p(t, stage).
// EVERY LDS read of the loop is inline asm, so hipcc counts none of them and the waits are written
// by hand.  LDS returns in order: `lgkmcnt(N)` retires all but the N youngest reads; each wait
// carries its fragments as "+v" operands, which orders the MFMAs that consume them behind it; the
// count argument stands next to each wait.  The counts hold only while hipcc puts nothing that
// counts on lgkmcnt, and no copy of a read's "=v" output, between a read and its wait: nothing
// enforces that, so re-read this loop in the -S output after a compiler upgrade (DESIGN 3b, Upkeep).
    static_assert(TI == 4, "the waits below name four A fragments per plane");
#define NAWS_PIPE_WAIT_A(N, AF) \
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(AF[0]), "+v"(AF[1]), "+v"(AF[2]), "+v"(AF[3]) : "n"(N));
#define NAWS_PIPE_WAIT_B(N, SET)                                                                \
  asm volatile("s_waitcnt lgkmcnt(%4)"                                                          \
               : "+v"(b[SET][0][0]), "+v"(b[SET][0][1]), "+v"(b[SET][1][0]), "+v"(b[SET][1][1]) \
               : "n"(N));
#define NAWS_PIPE_TERM(AF, BSET, SPH, Q)                                                        \
  _Pragma("unroll") for (int i = 0; i < TI; ++i) _Pragma("unroll") for (int jj = 0; jj < 2; ++jj) \
      acc[i][(SPH) * 2 + jj] = NAWS_PIPE_MFMA(b[BSET][Q][jj], AF[i], acc[i][(SPH) * 2 + jj]);
    // (the sched_barriers keep a sub-phase's reads in front of its MFMAs and out of the next one's)
#define NAWS_PIPE_MFMA01(CUR, BSET, SPH)  \
  __builtin_amdgcn_sched_barrier(0);      \
  NAWS_PIPE_TERM(a0[CUR], BSET, SPH, 0)   \
  NAWS_PIPE_TERM(a0[CUR], BSET, SPH, 1)
#define NAWS_PIPE_MFMA2(BSET, SPH)        \
  NAWS_PIPE_TERM(a1, BSET, SPH, 0)        \
  __builtin_amdgcn_sched_barrier(0);
    // CUR = TT & 1 (a literal): stage and a0 set of step TT.  In flight on entry: a0[CUR] (TI reads)
    // and B set 0 (NB) of this step, nothing else.
#define NAWS_PIPE_STEP(TT, CUR)                                                                 \
  NAWS_PIPE_READ_A(a1, 1, CUR)                                                                  \
  NAWS_PIPE_READ_B(1, CUR, 1)                                                                   \
  /* younger than a0 / B set 0: a1 (TI) + B set 1 (NB) */                                       \
  NAWS_PIPE_WAIT_A(TI + NAWS_PIPE_NB, a0[CUR])                                                  \
  NAWS_PIPE_WAIT_B(TI + NAWS_PIPE_NB, 0)                                                        \
  NAWS_PIPE_MFMA01(CUR, 0, 0)                                                                   \
  /* younger than a1: B set 1 (NB) */                                                           \
  __builtin_amdgcn_sched_barrier(0);                                                            \
  NAWS_PIPE_WAIT_A(NAWS_PIPE_NB, a1)                                                            \
  NAWS_PIPE_MFMA2(0, 0)                                                                         \
  _Pragma("unroll") for (int sp = 1; sp + 1 < SP; ++sp) {                                       \
    NAWS_PIPE_READ_B((sp + 1) & 1, CUR, sp + 1)                                                 \
    /* younger than B set sp: B set sp + 1 (NB) */                                              \
    NAWS_PIPE_WAIT_B(NAWS_PIPE_NB, sp & 1)                                                      \
    NAWS_PIPE_MFMA01(CUR, sp & 1, sp)                                                           \
    NAWS_PIPE_MFMA2(sp & 1, sp)                                                                 \
  }                                                                                             \
  /* the last B set: nothing younger; with it every read of this stage has retired */           \
  NAWS_PIPE_WAIT_B(0, (SP - 1) & 1)                                                             \
  if ((TT) + 1 < T) {                                                                           \
    wait_vmcnt<0>();          /* this wave's pieces of step TT + 1 (the only DMA in flight) */   \
    __builtin_amdgcn_s_barrier();                                                               \
    if ((TT) + 2 < T) issue_p((TT) + 2, CUR);                                                   \
    NAWS_PIPE_READ_A(a0[(CUR) ^ 1], 0, (CUR) ^ 1)                                               \
    NAWS_PIPE_READ_B(0, (CUR) ^ 1, 0)                                                           \
  }                                                                                             \
  NAWS_PIPE_MFMA01(CUR, (SP - 1) & 1, SP - 1)                                                   \
  NAWS_PIPE_MFMA2((SP - 1) & 1, SP - 1)
    issue_p(0, 0);
    if (T > 1) {
      issue_p(1, 1);
      wait_vmcnt<NAWS_PIPE_PIECES>();   // step 0's pieces landed, step 1's stay in flight
    } else {
      wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();
    NAWS_PIPE_READ_A(a0[0], 0, 0)
    NAWS_PIPE_READ_B(0, 0, 0)
    int t = 0;
    for (; t + 1 < T; t += 2) {
      NAWS_PIPE_STEP(t, 0)
      NAWS_PIPE_STEP(t + 1, 1)
    }
    if (t < T) {              // odd T: the last step (nothing to prefetch, no barrier)
      NAWS_PIPE_STEP(t, 0)
    }
#undef NAWS_PIPE_STEP
#undef NAWS_PIPE_MFMA2
#undef NAWS_PIPE_MFMA01
#undef NAWS_PIPE_TERM
#undef NAWS_PIPE_WAIT_B
#undef NAWS_PIPE_WAIT_A
