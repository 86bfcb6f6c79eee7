// Host-only argument front end of the GEMM and conv3x3 entry points (gemm_f32.hip, gemm_bf16.hip,
// gemm_x3.hip, gemm_btr.hip, conv_x3.hip): the checks and argument-struct fills every entry of a
// family repeats.  An entry point reads: family checks, its own conditions, fill, dispatch.  The
// ORDER of the checks is part of the ABI (it decides the code of a call that violates several
// conditions, tests/test_cabi.py pins it), so each helper covers one contiguous run of an entry's
// checks and the entries call them in their historical order.
#pragma once
#include "naws_common.h"

#define NAWS_TRY(expr)                 \
  do {                                 \
    const int rc_ = (expr);            \
    if (rc_ != NAWS_OK) return rc_;    \
  } while (0)

static inline bool naws_ptrs16(const void* a, const void* b = nullptr, const void* c = nullptr,
                               const void* d = nullptr, const void* e = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 15) == 0;
}

// ---- GEMM ------------------------------------------------------------------------------------------
// The epilogue triple: range, GATE_POS reads aux, the Dropout ratio lies in [0, 1).
static inline int naws_chk_epilogue(int epilogue, const float* aux, float drop_ratio) {
  if (epilogue < NAWS_EPI_NONE || epilogue > NAWS_EPI_GATE_POS) return NAWS_ERR_ARG;
  if (epilogue == NAWS_EPI_GATE_POS && aux == nullptr) return NAWS_ERR_NULL;
  if (epilogue == NAWS_EPI_BIAS_RELU_DROP && !(drop_ratio >= 0.f && drop_ratio < 1.f)) return NAWS_ERR_ARG;
  return NAWS_OK;
}

// Operand planes [plane][K/16][rows][16] of the _nt forms: a slab holds its rows, K is a multiple
// of the form's K-step `kmult` (16 / 32 / 64: the entry says which), every stride keeps the 16-byte
// DMA pieces aligned.  One-plane operands pass plane strides 0, unbatched ones batch strides 0.
static inline int naws_chk_planes_nt(int M, int N, int K, int kmult, const void* A, int64_t slabA,
                                     int64_t planeA, int64_t strideA, const void* B, int64_t slabB,
                                     int64_t planeB, int64_t strideB, int ldc) {
  if (slabA < (int64_t)M * 16 || slabB < (int64_t)N * 16 || ldc < N) return NAWS_ERR_SHAPE;
  if (K % kmult != 0 || slabA % 8 != 0 || slabB % 8 != 0 || planeA % 8 != 0 || planeB % 8 != 0 ||
      strideA % 8 != 0 || strideB % 8 != 0)
    return NAWS_ERR_ARG;
  if (!naws_ptrs16(A, B)) return NAWS_ERR_ARG;
  return NAWS_OK;
}

// The _xk forms (gemm_btr.hip) read X's FORWARD planes: what they require of K, N and the output's
// leading dimension is a property of the kernel (UNSUPPORTED), and comes before the null checks ...
static inline int naws_chk_xk_shape(int M, int N, int K, int xrows, int ld) {
  if (M <= 0 || N <= 0 || K <= 0 || xrows <= 0 || xrows > K) return NAWS_ERR_SHAPE;
  if (K % 32 != 0 || N % 16 != 0 || ld < N || ld % 4 != 0) return NAWS_ERR_UNSUPPORTED;
  return NAWS_OK;
}
// ... and their slab extents are argument errors, checked after the pointers' alignment (no % 8
// rules: these forms never had them).
static inline int naws_chk_planes_xk(int M, int xrows, const void* A, int64_t slabA, const void* X,
                                     int64_t slabX, const float* scaleX) {
  if (!naws_ptrs16(A, X, scaleX)) return NAWS_ERR_ARG;
  if (slabA < (int64_t)M * 16 || slabX < (int64_t)xrows * 16) return NAWS_ERR_ARG;
  return NAWS_OK;
}

// blockIdx.z carries the batch; C and aux are addressed with 32-bit element offsets.
static inline int naws_chk_batch_extent(int batch, int M, int N, int ldc, const float* aux, int ldaux) {
  if (batch > 65535) return NAWS_ERR_UNSUPPORTED;
  if ((long long)(M - 1) * ldc + N > 0x7fffffffLL ||
      (aux && (long long)(M - 1) * ldaux + N > 0x7fffffffLL))
    return NAWS_ERR_UNSUPPORTED;
  return NAWS_OK;
}

// The epilogue fields and batch strides of GemmArgs (gemm_f32.hip), BArgs (gemm_bf16.hip), XArgs.
template <class Args>
static inline void naws_fill_epilogue(Args& g, int epilogue, const float* bias, int64_t strideBias,
                                      const float* aux, int ldaux, float alpha, float drop_ratio,
                                      uint64_t seed, int accumulate, int64_t strideA, int64_t strideB,
                                      int64_t strideC) {
  g.sA = strideA; g.sB = strideB; g.sC = strideC; g.sBias = strideBias;
  g.bias = bias; g.aux = aux; g.ldaux = ldaux; g.alpha = alpha;
  g.drop_thr = naws_drop_threshold(drop_ratio);
  g.drop_scale = (float)(1.0 / (1.0 - (double)drop_ratio));
  g.seed = seed; g.epilogue = epilogue; g.accumulate = accumulate;
}

// The |C| maxima a GEMM epilogue reports.  A wave's columns must lie in one rowmax segment:
// segments are multiples of the widest tile (256), or cover all of N.
static inline int naws_fill_amax(NawsAmax& am, int M, int N, uint32_t* rowmax, int seg_cols,
                                 uint32_t* colmax, const float* colmul) {
  if (!rowmax && !colmax) return NAWS_OK;
  const int seg = seg_cols > 0 ? seg_cols : N;
  if (rowmax && seg < N && seg % 256 != 0) return NAWS_ERR_ARG;
  const int nseg = (int)naws_cdiv(N, seg);
  am.rowmax = rowmax; am.colmax = colmax; am.colmul = colmul;
  am.seg_cols = seg >= N ? 0x40000000 : seg;
  am.sRow = (long long)nseg * M; am.sCol = N;
  return NAWS_OK;
}

// ---- conv3x3 on weight planes (conv_x3.hip) -----------------------------------------------------------
// Between an entry's own shape / dilation / channel-multiple conditions and its dispatch, in two
// runs (the fp16x2 entry has conditions of its own between them): the pointers and "ReLU needs a
// bias" ...
static inline int naws_chk_conv_ptrs(const float* X, const void* Wp, const float* bias, int relu,
                                     const float* Y) {
  NAWS_REQUIRE_PTR(X); NAWS_REQUIRE_PTR(Wp); NAWS_REQUIRE_PTR(Y);
  if (!bias && relu) return NAWS_ERR_ARG;
  return NAWS_OK;
}
// ... then 16-byte operands, and a pixel count and input byte extent that fit 32-bit offsets.
static inline int naws_chk_conv_extent(const float* X, const void* Wp, int N, int H, int W, int Cin) {
  if (!naws_ptrs16(X, Wp)) return NAWS_ERR_ARG;
  const long long pix = (long long)N * H * W;
  if (pix > 0x7fffffffLL || pix * Cin * 4 > 0xFFFFFF00LL) return NAWS_ERR_UNSUPPORTED;
  return NAWS_OK;
}

// CArgs of a checked call: weight planes [planes][9 Cin / 16][Cout][16].
template <class Args>
static inline void naws_fill_conv(Args& g, const float* X, const void* Wp, const float* bias, float* Y,
                                  int N, int H, int W, int Cin, int Cout, int dilation, int relu) {
  const long long pix = (long long)N * H * W;
  g.X = X; g.B = (const unsigned short*)Wp; g.bias = bias; g.Y = Y;
  g.M = (int)pix; g.Cout = Cout; g.Cin = Cin; g.H = H; g.W = W; g.dil = dilation; g.relu = relu;
  g.slabB = (long long)Cout * 16;
  g.planeB = (long long)9 * Cin * Cout;
  g.bytesX = (unsigned)(pix * Cin * 4);
}
