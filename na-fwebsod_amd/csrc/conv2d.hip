// General NHWC convolution (kernel 1 / 3 / 7, stride 1 / 2, dilation 1 / 2) and AffineChannel: the
// two operators the ResNet18-WS body adds to the VGG-16 ones.
//   ref: detectron/modeling/ResNet18.py (add_ResNet18_conv{4,5}_body, residual_transformation) over
//        detectron/modeling/ResNet.py:203-256 (basic_bn_shortcut, basic_bn_stem); the operators are
//        Caffe2's built-in Conv and AffineChannel (pytorch v1.3.0 caffe2/operators), restated in
//        include/naws.h (a-1c) - that text is the contract.
//
// conv2d: implicit GEMM on the exact fp32-input MFMA (v_mfma_f32_16x16x4_f32): M = N*Ho*Wo output
// pixels, N = Cout, K = kernel*kernel*Cin in the order (kh, kw, ci) - the order of the packed weight
// [Cout][Kp], Kp = K rounded up to C2_KC with zeros.  One workgroup of 4 waves owns a 64-pixel x
// 64-channel tile and walks K in chunks of 32: every thread gathers two float4 of the im2col rows
// and two float4 of the weight rows into registers (the next chunk's loads are in flight while the
// current one is multiplied), stores them to LDS (rows padded to 36 floats: the fragment reads of a
// wave hit 64 different banks), and each wave multiplies its 32 x 32 quarter as 2 x 2 blocks of
// 16 x 16 with four independent accumulators.  The MFMA is issued with the operands swapped, so a
// lane holds 4 consecutive output channels of one pixel: the epilogue is one 16-byte NHWC store.
// With Cin % 32 == 0 a K chunk lies inside one tap and is 128 contiguous bytes of X; with Cin == 3
// (the 7x7 stem, K = 147) every element is gathered on its own and k >= K reads nothing.  A tap
// outside the image contributes 0, and its bounds are those of the pixel's own image: nothing of a
// neighbouring image is read.  Workgroups grid-stride over the M tiles (C2_MAX_GRID_M).
//
// affine_channel: memory-bound, NCHW, one float4 per lane over the flat tensor (the channel of
// every element is tracked, so H*W need not be a multiple of 4), scalar lanes for the tail; the
// product and the sum round separately (no FMA), so the result is bit-equal to x * s + b in fp32.
#include "naws_common.h"

namespace {

constexpr int C2_TB = 256;
constexpr int C2_BM = 64, C2_BN = 64, C2_KC = 32;
constexpr int C2_LD = C2_KC + 4;          // LDS row stride in floats (144 bytes: float4 rows stay aligned)
constexpr int C2_MAX_GRID_M = 1024;       // workgroups along M; the tiles beyond are grid-strided
constexpr int AC_TB = 256;
constexpr int AC_MAX_GRID = 256 * 16;

typedef float c2_f32x4 __attribute__((ext_vector_type(4)));

struct Conv2dArgs {
  const float* X;
  const float* Wp;
  const float* bias;
  float* Y;
  int N, H, W, Cin, Cout, Ho, Wo, kernel, stride, pad, dil, relu, K, Kp;
  int64_t M;
};

template <bool C3>
__global__ __launch_bounds__(C2_TB) void conv2d_kernel(const Conv2dArgs a) {
  __shared__ __attribute__((aligned(16))) float sA[C2_BM * C2_LD];
  __shared__ __attribute__((aligned(16))) float sB[C2_BN * C2_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, kg = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int n0 = blockIdx.y * C2_BN;
  const int lp = tid >> 3;                 // the row this thread stages (and lp + 32)
  const int kq = (tid & 7) * 4;            // its 4 k of the chunk
  const int64_t tiles = (a.M + C2_BM - 1) / C2_BM;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t m0 = tile * C2_BM;
    int py[2], px[2];
    int64_t pbase[2];
    bool pon[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int64_t m = m0 + lp + 32 * r;
      pon[r] = m < a.M;
      const int64_t mm = pon[r] ? m : 0;
      const int xo = (int)(mm % a.Wo);
      const int64_t t = mm / a.Wo;
      const int yo = (int)(t % a.Ho);
      const int n = (int)(t / a.Ho);
      py[r] = yo * a.stride - a.pad;
      px[r] = xo * a.stride - a.pad;
      pbase[r] = (int64_t)n * a.H * a.W;   // in pixels: the image's own rows only
    }
    float4 ra[2], rb[2];
    auto gload = [&](int k0) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int co = n0 + lp + 32 * r;
        rb[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (co < a.Cout)
          rb[r] = *reinterpret_cast<const float4*>(a.Wp + (int64_t)co * a.Kp + k0 + kq);
      }
      if constexpr (!C3) {
        const int tap = k0 / a.Cin;          // Cin % 32 == 0: the chunk lies inside one tap
        const int ci = k0 - tap * a.Cin + kq;
        const int kh = tap / a.kernel, kw = tap - kh * a.kernel;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int iy = py[r] + kh * a.dil, ix = px[r] + kw * a.dil;
          ra[r] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (pon[r] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
            ra[r] = *reinterpret_cast<const float4*>(
                a.X + (pbase[r] + (int64_t)iy * a.W + ix) * a.Cin + ci);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int k = k0 + kq + e;
            v[e] = 0.f;
            if (pon[r] && k < a.K) {
              const int tap = k / 3, ci = k - tap * 3;
              const int kh = tap / a.kernel, kw = tap - kh * a.kernel;
              const int iy = py[r] + kh * a.dil, ix = px[r] + kw * a.dil;
              if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                v[e] = a.X[(pbase[r] + (int64_t)iy * a.W + ix) * 3 + ci];
            }
          }
          ra[r] = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
    };
    c2_f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = c2_f32x4{0.f, 0.f, 0.f, 0.f};
    gload(0);
    for (int k0 = 0; k0 < a.Kp; k0 += C2_KC) {
      __syncthreads();                     // the previous chunk (or tile) has been read
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        *reinterpret_cast<float4*>(sA + (lp + 32 * r) * C2_LD + kq) = ra[r];
        *reinterpret_cast<float4*>(sB + (lp + 32 * r) * C2_LD + kq) = rb[r];
      }
      __syncthreads();
      if (k0 + C2_KC < a.Kp) gload(k0 + C2_KC);
#pragma unroll
      for (int ks = 0; ks < C2_KC / 4; ++ks) {
        float fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          fa[i] = sA[(wm * 32 + i * 16 + l15) * C2_LD + ks * 4 + kg];
          fb[i] = sB[(wn * 32 + i * 16 + l15) * C2_LD + ks * 4 + kg];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            // operands swapped: D[channel][pixel], so acc[i][j][e] = pixel l15, channel kg * 4 + e
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[j], fa[i], acc[i][j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t m = m0 + wm * 32 + i * 16 + l15;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = n0 + wn * 32 + j * 16 + kg * 4;
        if (m >= a.M || c >= a.Cout) continue;     // Cout % 4 == 0: a float4 is all in or all out
        c2_f32x4 v = acc[i][j];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (a.bias) v[e] += a.bias[c + e];
          if (a.relu) v[e] = fmaxf(v[e], 0.f);
        }
        *reinterpret_cast<c2_f32x4*>(a.Y + m * a.Cout + c) = v;
      }
    }
  }
}

__global__ __launch_bounds__(256) void conv2d_pack_kernel(const float* __restrict__ W, int Cout, int Cin,
                                                          int kernel, int K, int Kp,
                                                          float* __restrict__ Wp) {
  const int64_t total = (int64_t)Cout * Kp;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int k = (int)(t % Kp);
    const int co = (int)(t / Kp);
    float v = 0.f;
    if (k < K) {
      const int tap = k / Cin, ci = k - tap * Cin;
      const int kh = tap / kernel, kw = tap - kh * kernel;
      v = W[(((int64_t)co * Cin + ci) * kernel + kh) * kernel + kw];
    }
    Wp[t] = v;
  }
}

__device__ __forceinline__ float affine1(float x, float s, float b, int relu) {
#pragma clang fp contract(off)          // x * s rounds, then + b rounds: torch's x * s + b
  float y = x * s;
  y = y + b;
  return relu ? fmaxf(y, 0.f) : y;
}

// n4 float4 groups over the flat NCHW tensor, then the (total - 4 n4) tail elements one lane each
__global__ __launch_bounds__(AC_TB) void affine_channel_kernel(const float* X, const float* __restrict__ S,
                                                               const float* __restrict__ B, int C,
                                                               int64_t HW, int64_t total, int64_t n4,
                                                               int relu, float* Y) {
  const int64_t work = n4 + (total - 4 * n4);
  for (int64_t t = (int64_t)blockIdx.x * AC_TB + threadIdx.x; t < work;
       t += (int64_t)gridDim.x * AC_TB) {
    if (t < n4) {
      const int64_t i = 4 * t;
      const int64_t q = i / HW;
      int64_t r = i - q * HW;
      int c = (int)(q % C);
      const float4 x = *reinterpret_cast<const float4*>(X + i);
      float v[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = affine1(v[e], S[c], B[c], relu);
        if (++r == HW) {
          r = 0;
          if (++c == C) c = 0;
        }
      }
      *reinterpret_cast<float4*>(Y + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      const int64_t i = 4 * n4 + (t - n4);
      const int c = (int)((i / HW) % C);
      Y[i] = affine1(X[i], S[c], B[c], relu);
    }
  }
}

bool conv2d_args_ok(int kernel, int stride, int pad, int dilation) {
  if (kernel != 1 && kernel != 3 && kernel != 7) return false;
  if (stride != 1 && stride != 2) return false;
  if (dilation != 1 && dilation != 2) return false;
  return pad >= 0 && pad <= dilation * (kernel - 1);
}

}  // namespace

extern "C" int64_t naws_conv2d_packed_k(int Cin, int kernel) {
  if (Cin <= 0 || (kernel != 1 && kernel != 3 && kernel != 7)) return 0;
  return naws_cdiv((int64_t)kernel * kernel * Cin, C2_KC) * C2_KC;
}

extern "C" int naws_conv2d_max_grid_m(void) { return C2_MAX_GRID_M; }

extern "C" int naws_conv2d_pack_weight(const float* W_oihw, int Cout, int Cin, int kernel,
                                       float* Wp, void* stream) {
  if (Cout <= 0 || Cin <= 0) return NAWS_ERR_SHAPE;
  if (kernel != 1 && kernel != 3 && kernel != 7) return NAWS_ERR_ARG;
  if (Cout % 32 != 0 || (Cin != 3 && Cin % 32 != 0)) return NAWS_ERR_UNSUPPORTED;
  NAWS_REQUIRE_PTR(W_oihw); NAWS_REQUIRE_PTR(Wp);
  const int K = kernel * kernel * Cin;
  const int Kp = (int)naws_conv2d_packed_k(Cin, kernel);
  const int grid = (int)std::min<int64_t>(naws_cdiv((int64_t)Cout * Kp, 256), 2048);
  hipLaunchKernelGGL(conv2d_pack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, W_oihw, Cout,
                     Cin, kernel, K, Kp, Wp);
  return naws_check_launch();
}

extern "C" int naws_conv2d_nhwc_fwd(const float* X, const float* Wp, const float* bias, int N, int H,
                                    int W, int Cin, int Cout, int kernel, int stride, int pad,
                                    int dilation, int relu, float* Y, void* stream) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return NAWS_ERR_SHAPE;
  if (!conv2d_args_ok(kernel, stride, pad, dilation)) return NAWS_ERR_ARG;
  if (Cout % 32 != 0 || (Cin != 3 && Cin % 32 != 0)) return NAWS_ERR_UNSUPPORTED;
  const int eh = H + 2 * pad - dilation * (kernel - 1) - 1;
  const int ew = W + 2 * pad - dilation * (kernel - 1) - 1;
  if (eh < 0 || ew < 0) return NAWS_ERR_SHAPE;
  NAWS_REQUIRE_PTR(X); NAWS_REQUIRE_PTR(Wp); NAWS_REQUIRE_PTR(Y);
  if ((((uintptr_t)X | (uintptr_t)Wp | (uintptr_t)Y) % 16) != 0) return NAWS_ERR_ARG;
  Conv2dArgs a;
  a.X = X; a.Wp = Wp; a.bias = bias; a.Y = Y;
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
  a.Ho = eh / stride + 1; a.Wo = ew / stride + 1;
  a.kernel = kernel; a.stride = stride; a.pad = pad; a.dil = dilation; a.relu = relu;
  a.K = kernel * kernel * Cin;
  a.Kp = (int)naws_conv2d_packed_k(Cin, kernel);
  a.M = (int64_t)N * a.Ho * a.Wo;
  const dim3 grid((unsigned)std::min<int64_t>(naws_cdiv(a.M, C2_BM), C2_MAX_GRID_M),
                  (unsigned)naws_cdiv(Cout, C2_BN));
  if (Cin == 3)
    hipLaunchKernelGGL(conv2d_kernel<true>, grid, dim3(C2_TB), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(conv2d_kernel<false>, grid, dim3(C2_TB), 0, (hipStream_t)stream, a);
  return naws_check_launch();
}

extern "C" int naws_affine_channel_fwd(const float* X, const float* scale, const float* shift, int N,
                                       int C, int64_t HW, int relu, float* Y, void* stream) {
  if (N <= 0 || C <= 0 || HW <= 0) return NAWS_ERR_SHAPE;
  NAWS_REQUIRE_PTR(X); NAWS_REQUIRE_PTR(scale); NAWS_REQUIRE_PTR(shift); NAWS_REQUIRE_PTR(Y);
  const int64_t total = (int64_t)N * C * HW;
  // float4 lanes need both tensors on 16 bytes; otherwise every element goes through the tail
  const bool vec = (((uintptr_t)X | (uintptr_t)Y) % 16) == 0;
  const int64_t n4 = vec ? total / 4 : 0;
  const int64_t work = n4 + (total - 4 * n4);
  const int grid = (int)std::min<int64_t>(naws_cdiv(work, AC_TB), AC_MAX_GRID);
  hipLaunchKernelGGL(affine_channel_kernel, dim3(grid), dim3(AC_TB), 0, (hipStream_t)stream, X, scale,
                     shift, C, HW, total, n4, relu, Y);
  return naws_check_launch();
}
