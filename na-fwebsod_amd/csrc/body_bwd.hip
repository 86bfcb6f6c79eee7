// Backward of the conv body and of RoIPoolF for gfx950 (TRAIN.FREEZE_CONV_BODY False on the
// op-by-op plan): everything AROUND the two MFMA kernels the library already has.
//
//   dgrad  = naws_conv3x3_nhwc_fwd on dY with the flipped, transposed weight; this file packs it.
//   wgrad  = nine tap products X_shifted^T dY.  X and dY are staged zero-padded on one common
//            geometry (row width Wp = W + 2d, d zero rows above and below every image), so that
//            tap (ky,kx) is ONE strided GEMM whose A view starts ((ky-1) Wp + (kx-1)) d pixel rows
//            away from the B view: whatever a shifted pixel row reads outside its image is a
//            staged zero, or is multiplied by a staged zero of dY.  The products run on
//            naws_gemm_f32_splitk (fp32 MFMA, slices summed in a fixed order: dW is reproducible),
//            three taps (one ky) per batched call; one kernel then writes OIHW.
//   pool   = gather form of the 2x2 max-pool gradient, no atomics.
//   RoI    = scatter of dY through the forward's argmax with no-return float atomic adds
//            (global_atomic_add_f32), as the reference kernel does: the summation order of the
//            rois that share a pixel is not fixed, the result is reproducible to rounding only.
//
// ref: Caffe2 ConvGradient / MaxPoolGradient / RoIPoolFGradient (pytorch v1.3.0 caffe2/operators:
//      conv_op_impl.h, pool_gradient_op.cc, roi_pool_op.cu), detectron/modeling/VGG16.py:9-48.
#include "naws_common.h"

namespace {

constexpr int TB = 256;

inline int grid_for(int64_t n, int cap = 256 * 16) {
  return (int)std::min<int64_t>(std::max<int64_t>(naws_cdiv(n, TB), 1), cap);
}

// ---- RoIPoolF gradient -------------------------------------------------------------------------
// One thread per element of dY [R,C,nb]; argmax = h*W+w inside the (image, channel) plane or -1.
template <bool NHWC>
__global__ __launch_bounds__(TB) void roi_pool_bwd_kernel(
    const float* __restrict__ dY, const int32_t* __restrict__ argmax,
    const float* __restrict__ rois, int64_t total, int N, int C, int HW, int nb,
    float* __restrict__ dX) {
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * TB) {
    const int a = argmax[i];
    const int c = (int)((i / nb) % C);
    const int64_t r = i / ((int64_t)nb * C);
    const int b = (int)rois[r * 5];
    if ((unsigned)a >= (unsigned)HW || (unsigned)b >= (unsigned)N) continue;
    const int64_t o = NHWC ? ((int64_t)b * HW + a) * C + c : ((int64_t)b * C + c) * HW + a;
    unsafeAtomicAdd(dX + o, dY[i]);
  }
}

// ---- 2x2 max-pool gradient, NHWC, float4 lanes along channels ---------------------------------
// The forward takes fmaxf(fmaxf(a, b), fmaxf(d, e)) over a = (y,x), b = (y,x+1), d = (y+1,x),
// e = (y+1,x+1); the element it selects is the FIRST of a, b, d, e equal to that maximum.
__device__ __forceinline__ float pool_pick(float a, float b, float d, float e, float y, float g,
                                           int k) {
  // 1 when element k of the window is the selected one
  const float v = k == 0 ? a : (k == 1 ? b : (k == 2 ? d : e));
  bool sel = v == y;
  if (k > 0) sel = sel && a != y;
  if (k > 1) sel = sel && b != y;
  if (k > 2) sel = sel && d != y;
  return sel ? g : 0.f;
}

__global__ __launch_bounds__(TB) void maxpool2_bwd_kernel(
    const float4* __restrict__ X, const float4* __restrict__ Y, const float4* __restrict__ dY,
    int N, int H, int W, int C4, int stride, int Ho, int Wo, float4* __restrict__ dX) {
  const int64_t total = (int64_t)N * H * W * C4;
  for (int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * TB) {
    const int c = (int)(t % C4);
    const int w = (int)((t / C4) % W);
    const int h = (int)((t / ((int64_t)C4 * W)) % H);
    const int n = (int)(t / ((int64_t)C4 * W * H));
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    // windows (yo, xo) with yo*stride <= h <= yo*stride + 1, in ascending window index
    const int yo_lo = stride == 2 ? (h >> 1) : max(h - 1, 0);
    const int yo_hi = min(stride == 2 ? (h >> 1) : h, Ho - 1);
    const int xo_lo = stride == 2 ? (w >> 1) : max(w - 1, 0);
    const int xo_hi = min(stride == 2 ? (w >> 1) : w, Wo - 1);
    for (int yo = yo_lo; yo <= yo_hi; ++yo)
      for (int xo = xo_lo; xo <= xo_hi; ++xo) {
        const int y0 = yo * stride, x0 = xo * stride;
        const int k = (h - y0) * 2 + (w - x0);
        const float4* p = X + (((int64_t)n * H + y0) * W + x0) * C4 + c;
        const float4 a = p[0], b = p[C4], d = p[(int64_t)W * C4], e = p[(int64_t)W * C4 + C4];
        const int64_t o = (((int64_t)n * Ho + yo) * Wo + xo) * C4 + c;
        const float4 y = Y[o], g = dY[o];
        acc.x += pool_pick(a.x, b.x, d.x, e.x, y.x, g.x, k);
        acc.y += pool_pick(a.y, b.y, d.y, e.y, y.y, g.y, k);
        acc.z += pool_pick(a.z, b.z, d.z, e.z, y.z, g.z, k);
        acc.w += pool_pick(a.w, b.w, d.w, e.w, y.w, g.w, k);
      }
    dX[t] = acc;
  }
}

// ---- dgrad weight: OIHW -> packed [Cin][ky][kx][Cout] of W'[ci,co,ky,kx] = W[co,ci,2-ky,2-kx] ----
__global__ void dgrad_pack_kernel(const float* __restrict__ Wi, int Cout, int Cin,
                                  float* __restrict__ Wo) {
  const int64_t total = (int64_t)Cout * Cin * 9;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int co = (int)(i % Cout);
    const int tap = (int)((i / Cout) % 9);
    const int ci = (int)(i / ((int64_t)Cout * 9));
    Wo[i] = Wi[((int64_t)co * Cin + ci) * 9 + (8 - tap)];
  }
}

// ---- zero-padded staging: [N][H][W][C] -> [N][H+2d][W+2d][C] ---------------------------------
__global__ __launch_bounds__(TB) void pad_stage_kernel(const float4* __restrict__ S, int N, int H,
                                                       int W, int C4, int d,
                                                       float4* __restrict__ D) {
  const int Hp = H + 2 * d, Wp = W + 2 * d;
  const int64_t total = (int64_t)N * Hp * Wp * C4;
  for (int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * TB) {
    const int c = (int)(t % C4);
    const int x = (int)((t / C4) % Wp) - d;
    const int y = (int)((t / ((int64_t)C4 * Wp)) % Hp) - d;
    const int n = (int)(t / ((int64_t)C4 * Wp * Hp));
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (y >= 0 && y < H && x >= 0 && x < W) v = S[(((int64_t)n * H + y) * W + x) * C4 + c];
    D[t] = v;
  }
}

// ---- tap gradients T [9][Cin][Cout] -> dW [Cout][Cin][3][3] -----------------------------------
// 32 (ci) x 32 (co) tile of one tap through LDS: reads run along co, writes along ci.
__global__ void tap_repack_kernel(const float* __restrict__ T, int Cin, int Cout,
                                  float* __restrict__ dW) {
  __shared__ float tile[32][33];
  const int tap = blockIdx.z, ci0 = blockIdx.y * 32, co0 = blockIdx.x * 32;
  for (int i = threadIdx.y; i < 32; i += blockDim.y)
    tile[i][threadIdx.x] = T[((int64_t)tap * Cin + ci0 + i) * Cout + co0 + threadIdx.x];
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += blockDim.y)
    dW[((int64_t)(co0 + i) * Cin + ci0 + threadIdx.x) * 9 + tap] = tile[threadIdx.x][i];
}

struct WgradPlan {
  int d, Hp, Wp, ks;
  int64_t rows, p0, K;          // staged pixel rows; first valid pixel row; pixel rows the GEMM walks
  int64_t off_x, off_dy, off_t, off_part, floats;
};

// K slices: about 1024 workgroups over the 64 x 64 tiles of three taps, every slice >= 8 K-steps
WgradPlan wgrad_plan(int N, int H, int W, int Cin, int Cout, int d) {
  WgradPlan p;
  p.d = d; p.Hp = H + 2 * d; p.Wp = W + 2 * d;
  p.rows = (int64_t)N * p.Hp * p.Wp;
  p.p0 = (int64_t)d * p.Wp + d;
  p.K = p.rows - 2 * p.p0;      // up to the last valid pixel of the last image
  const int64_t tiles = naws_cdiv(Cin, 64) * naws_cdiv(Cout, 64) * 3;
  const int64_t steps = naws_cdiv(p.K, 32);
  p.ks = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(naws_cdiv(1024, tiles),
                                                                       steps / 8), 32));
  p.off_x = 0;
  p.off_dy = p.off_x + p.rows * Cin;
  p.off_t = p.off_dy + p.rows * Cout;
  p.off_part = p.off_t + (int64_t)9 * Cin * Cout;
  p.floats = p.off_part + (int64_t)Cin * Cout * 3 * p.ks;
  return p;
}

int wgrad_check(int N, int H, int W, int Cin, int Cout, int dilation) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return NAWS_ERR_SHAPE;
  if (dilation != 1 && dilation != 2) return NAWS_ERR_ARG;
  if (Cin % 32 != 0 || Cout % 32 != 0) return NAWS_ERR_UNSUPPORTED;
  return NAWS_OK;
}

}  // namespace

extern "C" int naws_roi_pool_f_bwd(const float* dY, const int32_t* argmax, const float* rois, int R,
                                   int layout, int N, int C, int H, int W, int pooled_h,
                                   int pooled_w, float* dX, void* stream) {
  if (R < 0 || N <= 0 || C <= 0 || H <= 0 || W <= 0 || pooled_h <= 0 || pooled_w <= 0)
    return NAWS_ERR_SHAPE;
  if (layout != NAWS_LAYOUT_NCHW && layout != NAWS_LAYOUT_NHWC) return NAWS_ERR_ARG;
  if ((int64_t)H * W > 0x7fffffffLL) return NAWS_ERR_UNSUPPORTED;
  NAWS_REQUIRE_PTR(dX);
  if (R > 0) { NAWS_REQUIRE_PTR(dY); NAWS_REQUIRE_PTR(argmax); NAWS_REQUIRE_PTR(rois); }
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(dX, 0, (size_t)N * C * H * W * sizeof(float), s);
  if (e != hipSuccess) {
    g_naws_last_hip_error = (int)e;
    return NAWS_ERR_LAUNCH;
  }
  if (R == 0) return NAWS_OK;
  const int nb = pooled_h * pooled_w;
  const int64_t total = (int64_t)R * C * nb;
  if (layout == NAWS_LAYOUT_NHWC)
    hipLaunchKernelGGL(roi_pool_bwd_kernel<true>, dim3(grid_for(total, 256 * 64)), dim3(TB), 0, s,
                       dY, argmax, rois, total, N, C, H * W, nb, dX);
  else
    hipLaunchKernelGGL(roi_pool_bwd_kernel<false>, dim3(grid_for(total, 256 * 64)), dim3(TB), 0, s,
                       dY, argmax, rois, total, N, C, H * W, nb, dX);
  return naws_check_launch();
}

extern "C" int naws_maxpool2x2_nhwc_bwd(const float* X, const float* Y, const float* dY, int N,
                                        int H, int W, int C, int stride, float* dX,
                                        void* stream) {
  if (N <= 0 || H < 2 || W < 2 || C <= 0) return NAWS_ERR_SHAPE;
  if (stride != 1 && stride != 2) return NAWS_ERR_ARG;
  NAWS_REQUIRE_PTR(X); NAWS_REQUIRE_PTR(Y); NAWS_REQUIRE_PTR(dY); NAWS_REQUIRE_PTR(dX);
  if (C % 4 != 0 || (((uintptr_t)X | (uintptr_t)Y | (uintptr_t)dY | (uintptr_t)dX) % 16) != 0)
    return NAWS_ERR_ARG;
  const int Ho = (H - 2) / stride + 1, Wo = (W - 2) / stride + 1;
  const int64_t total = (int64_t)N * H * W * (C / 4);
  hipLaunchKernelGGL(maxpool2_bwd_kernel, dim3(grid_for(total)), dim3(TB), 0, (hipStream_t)stream,
                     (const float4*)X, (const float4*)Y, (const float4*)dY, N, H, W, C / 4, stride,
                     Ho, Wo, (float4*)dX);
  return naws_check_launch();
}

extern "C" int naws_conv3x3_dgrad_pack_weight(const float* W_oihw, int Cout, int Cin,
                                              float* W_packed, void* stream) {
  if (Cout <= 0 || Cin <= 0) return NAWS_ERR_SHAPE;
  if (Cin % 32 != 0 || Cout % 32 != 0) return NAWS_ERR_UNSUPPORTED;
  NAWS_REQUIRE_PTR(W_oihw); NAWS_REQUIRE_PTR(W_packed);
  hipLaunchKernelGGL(dgrad_pack_kernel, dim3(grid_for((int64_t)Cout * Cin * 9, 256 * 8)), dim3(TB),
                     0, (hipStream_t)stream, W_oihw, Cout, Cin, W_packed);
  return naws_check_launch();
}

extern "C" int64_t naws_conv3x3_nhwc_wgrad_workspace_floats(int N, int H, int W, int Cin, int Cout,
                                                            int dilation) {
  if (wgrad_check(N, H, W, Cin, Cout, dilation) != NAWS_OK) return 0;
  return wgrad_plan(N, H, W, Cin, Cout, dilation).floats;
}

extern "C" int naws_conv3x3_nhwc_wgrad(const float* X, const float* dY, int N, int H, int W,
                                       int Cin, int Cout, int dilation, float* workspace,
                                       float* dW, float* db, void* stream) {
  const int rc0 = wgrad_check(N, H, W, Cin, Cout, dilation);
  if (rc0 != NAWS_OK) return rc0;
  NAWS_REQUIRE_PTR(X); NAWS_REQUIRE_PTR(dY); NAWS_REQUIRE_PTR(workspace); NAWS_REQUIRE_PTR(dW);
  NAWS_REQUIRE_PTR(db);
  if ((((uintptr_t)X | (uintptr_t)dY | (uintptr_t)workspace) % 16) != 0) return NAWS_ERR_ARG;
  const WgradPlan p = wgrad_plan(N, H, W, Cin, Cout, dilation);
  if (p.rows > 0x7fffffffLL) return NAWS_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int d = p.d;
  float* Xp = workspace + p.off_x;
  float* dYp = workspace + p.off_dy;
  float* T = workspace + p.off_t;
  float* part = workspace + p.off_part;
  hipLaunchKernelGGL(pad_stage_kernel, dim3(grid_for(p.rows * (Cin / 4))), dim3(TB), 0, s,
                     (const float4*)X, N, H, W, Cin / 4, d, (float4*)Xp);
  hipLaunchKernelGGL(pad_stage_kernel, dim3(grid_for(p.rows * (Cout / 4))), dim3(TB), 0, s,
                     (const float4*)dY, N, H, W, Cout / 4, d, (float4*)dYp);
  int rc = naws_check_launch();
  if (rc != NAWS_OK) return rc;
  // tap (ky, kx): T[tap] [Cin x Cout] = Xp[p0 + off .. + K)^T dYp[p0 .. + K), off = ((ky-1) Wp +
  // (kx-1)) d pixel rows; p0 + off >= 0 and p0 + off + K <= rows for all nine taps.  The three kx of
  // one ky are one batched call: A advances d pixel rows per item, B stays.
  for (int ky = 0; ky < 3; ++ky) {
    const int64_t off = ((int64_t)(ky - 1) * p.Wp - 1) * d;
    rc = naws_gemm_f32_splitk(1, 0, Cin, Cout, (int)p.K, Xp + (p.p0 + off) * Cin, Cin,
                              dYp + p.p0 * Cout, Cout, T + (int64_t)ky * 3 * Cin * Cout, Cout, 3,
                              (int64_t)d * Cin, 0, (int64_t)Cin * Cout, NAWS_EPI_NONE, nullptr, 0,
                              p.ks, part, stream);
    if (rc != NAWS_OK) return rc;
  }
  hipLaunchKernelGGL(tap_repack_kernel, dim3(Cout / 32, Cin / 32, 9), dim3(32, 8), 0, s,
                     (const float*)T, Cin, Cout, dW);
  rc = naws_check_launch();
  if (rc != NAWS_OK) return rc;
  return naws_colsum_f32(dY, (int)((int64_t)N * H * W), Cout, Cout, db, 0, stream);
}
