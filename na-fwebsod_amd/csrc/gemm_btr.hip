// fc6 weight gradient on the fp16x2 plan, reading the pooled features in their FORWARD layout.
//
//   dW[m][n] = sum_r dZ[r][m] x[r][n]        m < 8192 (both branches), n < 25088, r = proposal
//
// A = the transposing split of dZ (planes [2][R/16][M][16], K = r contiguous), as before.  B used
// to be a second copy of x: the RoIPool kernel writes x as the fc6 FORWARD operand, planes
// [2][n/16][r][16] (16 features of one proposal contiguous), and planes_transpose_kernel rewrote
// all 0.8 GB of it K-contiguous ([2][r/16][n][16]) once per step.  Here the GEMM takes the forward
// planes as they are: for a K-step of 32 proposals and a block of 16 features the forward layout
// holds 32 x 32 B = one contiguous KB - one LDS-DMA wave instruction, as many pieces per step as
// the K-contiguous form needs - and `ds_read_b64_tr_b16` reads it column-wise: per 16-lane group
// a block of 4 proposals x 16 features arrives feature-major, which IS the k-group of the
// 16x16x32 B operand (lane = feature, 4 consecutive k per read, two reads per fragment).
// LDS image of a (plane, 16-feature block): [32 proposal slots][32 B]; slot = proposal with bits 2
// and 3 swapped, so that the two 16-lane groups of a 32-lane half (k-groups kg, kg + 1) hit
// disjoint bank halves - conflict-free.  The swap is applied in the DMA's global source address
// (the DMA writes LDS lane-linearly).  Same tile (256 x 256, 4 x 2 waves of 64 x 128), ring,
// MFMA order and epilogue scaling as gemm_x3_m16_kernel: the accumulation order over k is the
// same, results are bit-identical to the transposed-copy route.
//
// replaces: FCGradient's dW for fc6 (reference detectron/modeling/wsl_heads.py:674-679 via
// Caffe2 FCGradient), with naws_f16_planes_transpose no longer on the path.
#include "x3_common.h"
#include "entry_args.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short i16x4 __attribute__((ext_vector_type(4)));

struct BArgs {
  const unsigned short* A;   // planes [2][K/16][M][16]
  const unsigned short* X;   // planes [2][N/16][xrows][16]
  float* C;
  int M, N, K, ldc, xrows;
  long long planeA, slabA, planeX, slabX;
  const float* rs;           // per-row factors undoing A's scaling
  const float* cs;           // per-column factors (null: 1)
  int tiles_m, tiles_n;
  // SGD form (naws_gemm_f32_f16x2_nt_xk_sgd): C is never written; the tile's products are the
  // gradient of param[M][ldp] and go straight into the update
  float* mom;
  float* param;
  int ldp;
  const float* lr;           // device scalar: the base learning rate
  float lr_mult, wd, momentum, gscale;
  int nesterov, first;
  unsigned short* P;         // param's fp16x2 operand planes [2][N/16][prows][16] (hi, then lo)
  long long planeP;
  int prows;
  const unsigned* bound;     // [M] max|param row| before this update (bit patterns)
  unsigned* rowmax;          // [M] max|param row| after it (atomic max; caller zeroes)
  float* inv_scale;          // [M]
  int* overflow;
  int overflow_tag;
};

// s_waitcnt lgkmcnt(0) that the fragments' consumers depend on (the asm reads are invisible to
// the compiler's own wait insertion)
template <int TJ>
__device__ __forceinline__ void frag_fence(f16x8 (&b)[TJ], bool wait) {
  static_assert(TJ == 8 || TJ == 4, "fragments per plane");
  if constexpr (TJ == 8) {
    if (wait)
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7]));
    else
      asm volatile("" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7]));
  } else {
    if (wait)
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
    else
      asm volatile("" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
  }
}

constexpr int KS = 2, NPL = 2, STAGES = 2, NQ = NPL * KS;

// <256, 256, 4, 2>: 512 threads, waves of 64 x 128;  <128, 128, 2, 2>: 256 threads, waves of 64 x 64
// (the last column tiles of a problem whose tile count is not a multiple of the CU count)
template <int BM, int BN, int WM, int WN, bool SGD = false>
__global__ __launch_bounds__(64 * WM * WN, (WM * WN >= 8 ? 1 : 2)) void gemm_h2_btr_kernel(BArgs g) {
#define NAWS_BTR_PIPE false
#include "gemm_btr_body.inc"
#undef NAWS_BTR_PIPE
}

// the same tile, epilogues and accumulation order behind the software-pipelined K loop
template <int BM, int BN, int WM, int WN, bool SGD = false>
__global__ __launch_bounds__(64 * WM * WN, (WM * WN >= 8 ? 1 : 2)) void gemm_h2_btrp_kernel(BArgs g) {
#define NAWS_BTR_PIPE true
#include "gemm_btr_body.inc"
#undef NAWS_BTR_PIPE
}

template <int BM, int BN, int WM, int WN, bool SGD = false, bool PIPE = false>
int launch_btr(BArgs& g, hipStream_t s) {
  g.tiles_m = (int)naws_cdiv(g.M, BM);
  g.tiles_n = (int)naws_cdiv(g.N, BN);
  void (*kern)(BArgs) = gemm_h2_btr_kernel<BM, BN, WM, WN, SGD>;
  if constexpr (PIPE) kern = gemm_h2_btrp_kernel<BM, BN, WM, WN, SGD>;
  if (naws_allow_lds(kern) != NAWS_OK) return NAWS_ERR_LAUNCH;
  hipLaunchKernelGGL(kern, dim3((unsigned)(g.tiles_m * g.tiles_n)), dim3(64 * WM * WN),
                     (size_t)STAGES * NQ * (BM + BN) * 32, s, g);
  return naws_check_launch();
}

// h2 = 18 / 19 (gemm_x3.hip): the two-phase K loop in the 256 x 256 form, for the in-process A/B and
// the bit-identity tests; otherwise the software-pipelined loop
bool btr_two_phase() {
  const int v = naws_knob(NAWS_KNOB_H2);
  return v == 18 || v == 19;
}

// the operand fields both entry points share (ld = ldc, or ldp in the SGD form)
void fill_btr(BArgs& g, int M, int N, int K, const void* A2, int64_t slabA, int64_t planeA,
              const float* scaleA, const void* X2, int64_t slabX, int64_t planeX, int xrows,
              const float* scaleX, float* C, int ld) {
  g.A = (const unsigned short*)A2; g.X = (const unsigned short*)X2; g.C = C;
  g.M = M; g.N = N; g.K = K; g.ldc = ld; g.xrows = xrows;
  g.planeA = planeA; g.slabA = slabA; g.planeX = planeX; g.slabX = slabX;
  g.rs = scaleA; g.cs = scaleX;
}

}  // namespace

// C [M x N] (ld ldc) = A^T-planes x X-planes: A2 = planes [2][K/16][M][16] with per-row factors
// scaleA; X2 = planes [2][N/16][xrows][16] (the forward operand of an [xrows x N] matrix, e.g.
// naws_roi_pool_f_f16x2_fwd's output), k = its row index, scaleX per column (nullable: ones).
// K % 32 == 0 (A's planes zero-padded beyond the xrows valid proposals), N % 16 == 0.
extern "C" int naws_gemm_f32_f16x2_nt_xk(int M, int N, int K, const void* A2, int64_t slabA,
                                         int64_t planeA, const float* scaleA, const void* X2,
                                         int64_t slabX, int64_t planeX, int xrows,
                                         const float* scaleX, float* C, int ldc, void* stream) {
  NAWS_TRY(naws_chk_xk_shape(M, N, K, xrows, ldc));
  NAWS_REQUIRE_PTR(A2); NAWS_REQUIRE_PTR(X2); NAWS_REQUIRE_PTR(scaleA); NAWS_REQUIRE_PTR(C);
  if (!naws_ptrs16(C)) return NAWS_ERR_ARG;
  NAWS_TRY(naws_chk_planes_xk(M, xrows, A2, slabA, X2, slabX, scaleX));
  BArgs g{};
  fill_btr(g, M, N, K, A2, slabA, planeA, scaleA, X2, slabX, planeX, xrows, scaleX, C, ldc);
  hipStream_t s = (hipStream_t)stream;
  // few tiles (the column remainder of fc6's dW): 128 x 128 tiles, two workgroups per CU
  if (naws_cdiv(M, 256) * naws_cdiv(N, 256) < 256) return launch_btr<128, 128, 2, 2>(g, s);
  if (btr_two_phase()) return launch_btr<256, 256, 4, 2>(g, s);
  return launch_btr<256, 256, 4, 2, false, true>(g, s);
}

// The same product with the ACM SGD update of `param` (an [M x N] block, ld ldp, of the parameter
// arena; `mom` its momentum) in the epilogue instead of the store: the gradient
// g = A^T-planes x X-planes never reaches memory.  For a run WITHOUT a gradient exchange (one
// process: the reference adds its all-reduce ops only when NUM_GPUS > 1,
// detectron/modeling/optimizer_wsl.py:52-72); with more ranks the gradient must be written,
// reduced and then applied (naws_acm_sgd_update_f16x2).  Element arithmetic, scale bound, maxima
// and overflow word exactly as naws_acm_sgd_update_f16x2 applies them to a region (head_ops.hip):
// parameters, momentum and planes come out bit-identical to the two-kernel route.
// replaces: FCGradient's dW for fc6 + ACMWeightDecayMomentumSGDUpdate on fc6_w
// (reference detectron/ops/acm_weightdecay_momentum_sgd_op.h:72-109), ITER_SIZE 1.
extern "C" int naws_gemm_f32_f16x2_nt_xk_sgd(
    int M, int N, int K, const void* A2, int64_t slabA, int64_t planeA, const float* scaleA,
    const void* X2, int64_t slabX, int64_t planeX, int xrows, const float* scaleX, float* param,
    float* momentum_buf, int ldp, const float* lr, float lr_mult, float weight_decay, float momentum,
    int nesterov, int gpu_num, int64_t iter_count, void* planes, int64_t plane_stride,
    int plane_rows, const uint32_t* bound, uint32_t* rowmax, float* inv_scale, int32_t* overflow,
    int32_t overflow_tag, void* stream) {
  if (gpu_num <= 0 || iter_count < 0 || plane_rows <= 0) return NAWS_ERR_SHAPE;
  NAWS_TRY(naws_chk_xk_shape(M, N, K, xrows, ldp));
  NAWS_REQUIRE_PTR(A2); NAWS_REQUIRE_PTR(X2); NAWS_REQUIRE_PTR(scaleA); NAWS_REQUIRE_PTR(param);
  NAWS_REQUIRE_PTR(momentum_buf); NAWS_REQUIRE_PTR(lr); NAWS_REQUIRE_PTR(planes);
  NAWS_REQUIRE_PTR(bound); NAWS_REQUIRE_PTR(rowmax); NAWS_REQUIRE_PTR(inv_scale);
  NAWS_REQUIRE_PTR(overflow);
  if (!naws_ptrs16(param, momentum_buf)) return NAWS_ERR_ARG;
  if (((uintptr_t)planes & 7) != 0 || (const void*)bound == (const void*)rowmax) return NAWS_ERR_ARG;
  NAWS_TRY(naws_chk_planes_xk(M, xrows, A2, slabA, X2, slabX, scaleX));
  if (plane_rows < M) return NAWS_ERR_ARG;      // the block lies inside one batch item of the planes
  BArgs g{};
  fill_btr(g, M, N, K, A2, slabA, planeA, scaleA, X2, slabX, planeX, xrows, scaleX, nullptr, ldp);
  g.mom = momentum_buf; g.param = param; g.ldp = ldp; g.lr = lr; g.lr_mult = lr_mult;
  g.wd = weight_decay; g.momentum = momentum; g.gscale = (float)(1.0 / (double)gpu_num);
  g.nesterov = nesterov; g.first = iter_count == 0 ? 1 : 0;
  g.P = (unsigned short*)planes; g.planeP = plane_stride; g.prows = plane_rows;
  g.bound = bound; g.rowmax = rowmax; g.inv_scale = inv_scale; g.overflow = overflow;
  g.overflow_tag = overflow_tag;
  hipStream_t s = (hipStream_t)stream;
  if (naws_cdiv(M, 256) * naws_cdiv(N, 256) < 256) return launch_btr<128, 128, 2, 2, true>(g, s);
  if (btr_two_phase()) return launch_btr<256, 256, 4, 2, true>(g, s);
  return launch_btr<256, 256, 4, 2, true, true>(g, s);
}
