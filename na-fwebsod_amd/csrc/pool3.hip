// MaxPool kernel 3 / pad 1 / stride 1 or 2, NHWC (the pools of the DeepLab VGG-16 body).
//   ref: detectron/modeling/VGG16.py:94-140 (`add_VGG16_conv5_body_deeplab`: pool1..pool3 at
//        stride 2, pool4 at stride 1 under WSL.DILATION 2); the operator is Caffe2's built-in
//        MaxPool (pytorch v1.3.0 caffe2/operators/pool_op.cc, legacy floor output size), restated
//        in include/naws.h - that text is the contract, no reference-executed number pins it.
//
// Memory-bound: lanes run along C (one float4 = 16 bytes per lane, a wave reads and writes whole
// 256-byte runs), and one thread owns P3_PX consecutive output pixels of a row.  It reduces each
// input column of its strip over the (clipped) three rows first, then every output over its
// (clipped) three columns: 3 * ((P3_PX - 1) * stride + 3) loads for P3_PX outputs - 18 instead of
// 36 at stride 1, 27 instead of 36 at stride 2; the rows shared with the strips above and below
// come from L1 / L2.  No LDS.  Padding is never a candidate: the centre row and the centre column
// of a window always lie inside the image, the reduction starts from them and a clipped column
// carries -inf, which the centre column then replaces.
#include <math.h>
#include "naws_common.h"

namespace {

constexpr int P3_TB = 256;
constexpr int P3_PX = 4;            // output pixels of one row per thread
constexpr int P3_MAX_GRID = 256 * 16;

__device__ __forceinline__ float4 max4(const float4 a, const float4 b) {
  return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}

template <int S>
__global__ __launch_bounds__(P3_TB) void maxpool3_kernel(const float4* __restrict__ X, int N, int H,
                                                         int W, int C4, int Ho, int Wo, int Wseg,
                                                         float4* __restrict__ Y) {
  constexpr int NCOL = (P3_PX - 1) * S + 3;
  const int64_t total = (int64_t)N * Ho * Wseg * C4;
  for (int64_t t = (int64_t)blockIdx.x * P3_TB + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * P3_TB) {
    const int c = (int)(t % C4);
    const int xs = (int)((t / C4) % Wseg);
    const int yo = (int)((t / ((int64_t)C4 * Wseg)) % Ho);
    const int n = (int)(t / ((int64_t)C4 * Wseg * Ho));
    const int y = yo * S;                       // the centre row: 0 <= y <= H - 1
    const int xo0 = xs * P3_PX;
    const int x0 = xo0 * S - 1;                 // the strip's first input column (may be -1)
    const bool up = y > 0, down = y + 1 < H;
    const float4* row = X + ((int64_t)n * H + y) * W * C4 + c;
    const int64_t rs = (int64_t)W * C4;
    float4 col[NCOL];
#pragma unroll
    for (int j = 0; j < NCOL; ++j) {
      const int x = x0 + j;
      float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      if (x >= 0 && x < W) {
        const float4* p = row + (int64_t)x * C4;
        m = p[0];
        if (up) m = max4(m, p[-rs]);
        if (down) m = max4(m, p[rs]);
      }
      col[j] = m;
    }
    float4* out = Y + (((int64_t)n * Ho + yo) * Wo + xo0) * C4 + c;
#pragma unroll
    for (int k = 0; k < P3_PX; ++k)
      if (xo0 + k < Wo)
        out[(int64_t)k * C4] = max4(col[k * S + 1], max4(col[k * S], col[k * S + 2]));
  }
}

}  // namespace

extern "C" int naws_maxpool3x3_nhwc_fwd(const float* X, int N, int H, int W, int C, int stride,
                                        float* Y, void* stream) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return NAWS_ERR_SHAPE;
  if (stride != 1 && stride != 2) return NAWS_ERR_ARG;
  if (C % 4 != 0 || (((uintptr_t)X | (uintptr_t)Y) % 16) != 0) return NAWS_ERR_ARG;
  NAWS_REQUIRE_PTR(X); NAWS_REQUIRE_PTR(Y);
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;   // (H + 2 - 3) / stride + 1
  const int Wseg = (int)naws_cdiv(Wo, P3_PX);
  const int64_t total = (int64_t)N * Ho * Wseg * (C / 4);
  const int grid = (int)std::min<int64_t>(naws_cdiv(total, P3_TB), P3_MAX_GRID);
  if (stride == 1)
    hipLaunchKernelGGL(maxpool3_kernel<1>, dim3(grid), dim3(P3_TB), 0, (hipStream_t)stream,
                       (const float4*)X, N, H, W, C / 4, Ho, Wo, Wseg, (float4*)Y);
  else
    hipLaunchKernelGGL(maxpool3_kernel<2>, dim3(grid), dim3(P3_TB), 0, (hipStream_t)stream,
                       (const float4*)X, N, H, W, C / 4, Ho, Wo, Wseg, (float4*)Y);
  return naws_check_launch();
}
