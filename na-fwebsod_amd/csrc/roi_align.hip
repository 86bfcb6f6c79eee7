// RoIAlign / RoIAlignGradient (FAST_RCNN.ROI_XFORM_METHOD RoIAlign), NHWC features.
//   ref: detectron/modeling/detector.py:268-331 (op emission); the operator is Caffe2's built-in
//        (pytorch v1.3.0 caffe2/operators/roi_align_op.cc, roi_align_gradient_op.cu, aligned =
//        false), restated in include/naws.h - that text is the contract, no reference-executed
//        number pins it.
//
// The average of a bilinear interpolant over a bin's sample grid is linear and separable in the
// pixels:
//     Y[c,p,q] = sum_h sum_w Ay[p,h] Ax[q,w] X[h,w,c]
// with Ay[p,h] = (the summed row weights of bin p's samples on row h) / gh, Ax likewise.  One
// workgroup = one roi x RA_WAVES channel tiles of 64: it builds Ay [ph][H] and Ax [pw][W] once in
// LDS (one lane per bin, samples in ascending order), then every wave walks the rows and columns
// that carry a weight with its 64 lanes on 64 contiguous channels - each X read and each dX add is
// one 256-byte line, each pixel is visited once per bin column it feeds, not once per sample tap.
// Per row / column the first and last bin that feeds it are kept too (the weights form a band), so
// the inner loops run over one or two bins, not over all of them.
//   forward : t = sum_w Ax[q,w] X[h,w,c] in a register, Y[p,q] += Ay[p,h] t in a per-lane LDS
//             column; rows, bins and columns ascend, so Y is bit-reproducible.  The 64 x ph*pw
//             tile leaves through LDS (row stride 65 floats: lanes over channels write
//             conflict-free, lanes over the output run read at most 2-way) as ONE contiguous run
//             Y[r, c0:c0+64].
//   backward: u[q] = sum_p Ay[p,h] dY[c,p,q] per row, g = sum_q Ax[q,w] u[q] per pixel, then ONE
//             no-return float atomic add per (pixel, channel): 256 contiguous bytes per wave
//             instruction.  Rois that share a pixel add in no fixed order.
// Only the geometry (sample coordinates, validity, taps, l) is defined to the bit: those
// functions switch contraction off (the library builds with -ffp-contract=fast-honor-pragmas).
#include <float.h>
#include <math.h>
#include "naws_common.h"

namespace {

constexpr int RA_WAVES = 4;               // channel tiles per workgroup (they share the tables)
constexpr int RA_TB = RA_WAVES * NAWS_WAVE;
constexpr int RA_STRIDE = NAWS_WAVE + 1;  // floats between two bins of a wave's staging tile
constexpr int RA_MAX_GRID = 1024;         // cap of an ADAPTIVE sample grid (include/naws.h)

struct RaFrame {
  int batch, gh, gw;
  float ys, xs, bh, bw;
};

// The roi's frame, every operation one fp32 operation.  false = the roi is invalid as a whole.
__device__ __forceinline__ bool ra_frame(const float* __restrict__ roi, float s, int N, int PH,
                                         int PW, int sampling, RaFrame& f) {
#pragma clang fp contract(off)
  const float bf = roi[0];
  if (!(bf > -1.0f && bf < (float)N)) return false;      // (int) truncates; a NaN fails too
  f.batch = (int)bf;
  f.xs = roi[1] * s; f.ys = roi[2] * s;
  const float xe = roi[3] * s, ye = roi[4] * s;
  if (!(fabsf(f.xs) <= FLT_MAX && fabsf(f.ys) <= FLT_MAX && fabsf(xe) <= FLT_MAX &&
        fabsf(ye) <= FLT_MAX))
    return false;
  const float rw = fmaxf(xe - f.xs, 1.0f), rh = fmaxf(ye - f.ys, 1.0f);
  f.bw = rw / (float)PW;
  f.bh = rh / (float)PH;
  if (sampling > 0) {
    f.gh = f.gw = sampling;
  } else {
    const float gwf = ceilf(rw / (float)PW), ghf = ceilf(rh / (float)PH);
    if (!(gwf <= (float)RA_MAX_GRID && ghf <= (float)RA_MAX_GRID)) return false;   // inf too
    f.gw = (int)gwf; f.gh = (int)ghf;
  }
  return true;
}

// Sample i of bin p on one axis of length L.  lo, hi are always inside [0, L).
__device__ __forceinline__ bool ra_sample(float start, float bin, int g, int p, int i, int L, int& lo,
                                          int& hi, float& l) {
#pragma clang fp contract(off)
  float y = (start + (float)p * bin) + (((float)i + 0.5f) * bin) / (float)g;
  if (!(y >= -1.0f && y <= (float)L)) return false;
  if (y <= 0.0f) y = 0.0f;
  lo = (int)y;
  if (lo >= L - 1) {
    hi = lo = L - 1;
    y = (float)lo;
  } else {
    hi = lo + 1;
  }
  l = y - (float)lo;
  return true;
}

// LDS image of a workgroup: [Ay ph*H][Ax pw*W][rp0 H][rp1 H][cq0 W][cq1 W][q0 pw][q1 pw][box 4]
// then per wave [tile nb*65] (+ [u pw*64] in the backward).  The weights form a band: row h is fed
// by the bins rp0[h]..rp1[h] only (rp1 < 0: by none), column w by cq0[w]..cq1[w]; bin column q
// reads the columns q0[q]..q1[q].
struct RaTables {
  float* Ay; float* Ax;
  int* rp0; int* rp1; int* cq0; int* cq1; int* q0; int* q1; int* box;   // box: hmin, hmax, wmin, wmax
  float* waves;
};

__device__ __forceinline__ RaTables ra_carve(float* smem, int PH, int PW, int H, int W) {
  RaTables t;
  t.Ay = smem;
  t.Ax = t.Ay + PH * H;
  t.rp0 = reinterpret_cast<int*>(t.Ax + PW * W);
  t.rp1 = t.rp0 + H;
  t.cq0 = t.rp1 + H;
  t.cq1 = t.cq0 + W;
  t.q0 = t.cq1 + W;
  t.q1 = t.q0 + PW;
  t.box = t.q1 + PW;
  t.waves = reinterpret_cast<float*>(t.box + 4);
  return t;
}

size_t ra_table_floats(int PH, int PW, int H, int W) {
  return (size_t)PH * H + (size_t)PW * W + 2 * ((size_t)H + W) + 2 * (size_t)PW + 4;
}

// Builds the tables of roi `roi`; returns (to every thread) whether the roi is valid.  Ends on a
// barrier.  One lane per bin adds its samples' weights in ascending sample order.
__device__ bool ra_build(const RaTables& t, const float* __restrict__ roi, float s, int N, int PH,
                         int PW, int H, int W, int sampling, int& batch) {
  RaFrame f;
  const int tid = threadIdx.x;
  const bool valid = ra_frame(roi, s, N, PH, PW, sampling, f);   // uniform: every thread computes it
  batch = valid ? f.batch : 0;
  if (valid) {
    for (int i = tid; i < PH * H + PW * W; i += RA_TB) t.Ay[i] = 0.0f;   // Ax follows Ay
    if (tid < 4) t.box[tid] = (tid & 1) ? -1 : 0x7fffffff;
    __syncthreads();
    for (int b = tid; b < PH + PW; b += RA_TB) {
      const bool row = b < PH;
      const int p = row ? b : b - PH;
      const int L = row ? H : W, g = row ? f.gh : f.gw;
      const float start = row ? f.ys : f.xs, bin = row ? f.bh : f.bw;
      float* A = row ? t.Ay + (size_t)p * H : t.Ax + (size_t)p * W;
      int first = 0x7fffffff, last = -1;
      for (int i = 0; i < g; ++i) {
        int lo, hi;
        float l;
        if (!ra_sample(start, bin, g, p, i, L, lo, hi, l)) continue;
        A[lo] += 1.0f - l;
        A[hi] += l;
        first = min(first, lo);
        last = max(last, hi);
      }
      if (!row) { t.q0[p] = first; t.q1[p] = last; }
    }
    __syncthreads();
    // divide by the grid count; the band of bins that feeds each row / column, and their box
    const float ngh = (float)f.gh, ngw = (float)f.gw;
    for (int h = tid; h < H; h += RA_TB) {
      int lo = PH, hi = -1;
      for (int p = 0; p < PH; ++p) {
        const float a = t.Ay[(size_t)p * H + h] / ngh;
        t.Ay[(size_t)p * H + h] = a;
        if (a != 0.0f) { lo = min(lo, p); hi = p; }
      }
      t.rp0[h] = lo; t.rp1[h] = hi;
      if (hi >= 0) { atomicMin(&t.box[0], h); atomicMax(&t.box[1], h); }
    }
    for (int w = tid; w < W; w += RA_TB) {
      int lo = PW, hi = -1;
      for (int q = 0; q < PW; ++q) {
        const float a = t.Ax[(size_t)q * W + w] / ngw;
        t.Ax[(size_t)q * W + w] = a;
        if (a != 0.0f) { lo = min(lo, q); hi = q; }
      }
      t.cq0[w] = lo; t.cq1[w] = hi;
      if (hi >= 0) { atomicMin(&t.box[2], w); atomicMax(&t.box[3], w); }
    }
  }
  __syncthreads();
  return valid;
}

__global__ __launch_bounds__(RA_TB) void roi_align_fwd_kernel(
    const float* __restrict__ X, int N, int C, int H, int W, const float* __restrict__ rois, int PH,
    int PW, float s, int sampling, float* __restrict__ Y) {
  extern __shared__ float ra_smem[];
  const RaTables t = ra_carve(ra_smem, PH, PW, H, W);
  const int r = blockIdx.x, nb = PH * PW;
  const int wave = threadIdx.x / NAWS_WAVE, lane = threadIdx.x % NAWS_WAVE;
  const int c0 = (blockIdx.y * RA_WAVES + wave) * NAWS_WAVE;
  const int c = c0 + lane;
  const bool live = c0 < C, cvalid = c < C;
  float* tile = t.waves + (size_t)wave * nb * RA_STRIDE;
  int batch;
  const bool valid = ra_build(t, rois + (size_t)r * 5, s, N, PH, PW, H, W, sampling, batch);
  if (live)
    for (int j = 0; j < nb; ++j) tile[j * RA_STRIDE + lane] = 0.0f;
  if (valid && live) {
    const int h0 = t.box[0], h1 = t.box[1];
    const float* Xb = X + (size_t)batch * H * W * C + (cvalid ? c : c0);   // masked lanes stay inside
    for (int h = h0; h <= h1; ++h) {
      const int p0 = t.rp0[h], p1 = t.rp1[h];
      if (p1 < 0) continue;
      const float* xrow = Xb + (size_t)h * W * C;
      for (int q = 0; q < PW; ++q) {
        const int w0 = t.q0[q], w1 = t.q1[q];
        if (w1 < w0) continue;      // no valid sample in this bin column
        const float* ax = t.Ax + (size_t)q * W;
        float acc = 0.0f;
        for (int w = w0; w <= w1; ++w) {
          const float a = ax[w];
          if (a != 0.0f) acc += a * xrow[(size_t)w * C];
        }
        for (int p = p0; p <= p1; ++p) {
          const float a = t.Ay[(size_t)p * H + h];
          if (a != 0.0f) tile[(p * PW + q) * RA_STRIDE + lane] += a * acc;
        }
      }
    }
  }
  __syncthreads();
  if (live) {
    const int run = min(NAWS_WAVE, C - c0) * nb;
    float* y = Y + ((size_t)r * C + c0) * nb;
    for (int e = lane; e < run; e += NAWS_WAVE) y[e] = tile[(e % nb) * RA_STRIDE + e / nb];
  }
}

__global__ __launch_bounds__(RA_TB) void roi_align_bwd_kernel(
    const float* __restrict__ dY, const float* __restrict__ rois, int N, int C, int H, int W, int PH,
    int PW, float s, int sampling, float* __restrict__ dX) {
  extern __shared__ float ra_smem[];
  const RaTables t = ra_carve(ra_smem, PH, PW, H, W);
  const int r = blockIdx.x, nb = PH * PW;
  const int wave = threadIdx.x / NAWS_WAVE, lane = threadIdx.x % NAWS_WAVE;
  const int c0 = (blockIdx.y * RA_WAVES + wave) * NAWS_WAVE;
  const int c = c0 + lane;
  const bool live = c0 < C, cvalid = c < C;
  float* tile = t.waves + (size_t)wave * (nb * RA_STRIDE + PW * NAWS_WAVE);
  float* u = tile + (size_t)nb * RA_STRIDE;
  int batch;
  const bool valid = ra_build(t, rois + (size_t)r * 5, s, N, PH, PW, H, W, sampling, batch);
  if (valid && live) {
    const int run = min(NAWS_WAVE, C - c0) * nb;
    const float* dy = dY + ((size_t)r * C + c0) * nb;
    for (int e = lane; e < run; e += NAWS_WAVE) tile[(e % nb) * RA_STRIDE + e / nb] = dy[e];
  }
  __syncthreads();
  if (valid && live) {
    const int h0 = t.box[0], h1 = t.box[1], w0 = t.box[2], w1 = t.box[3];
    float* dXb = dX + (size_t)batch * H * W * C + (cvalid ? c : c0);
    for (int h = h0; h <= h1; ++h) {
      const int p0 = t.rp0[h], p1 = t.rp1[h];
      if (p1 < 0) continue;
      for (int q = 0; q < PW; ++q) {
        float acc = 0.0f;
        for (int p = p0; p <= p1; ++p) {
          const float a = t.Ay[(size_t)p * H + h];
          if (a != 0.0f && cvalid) acc += a * tile[(p * PW + q) * RA_STRIDE + lane];
        }
        u[q * NAWS_WAVE + lane] = acc;
      }
      float* drow = dXb + (size_t)h * W * C;
      for (int w = w0; w <= w1; ++w) {
        const int qa = t.cq0[w], qb = t.cq1[w];
        if (qb < 0) continue;
        float g = 0.0f;
        for (int q = qa; q <= qb; ++q) {
          const float a = t.Ax[(size_t)q * W + w];
          if (a != 0.0f) g += a * u[q * NAWS_WAVE + lane];
        }
        if (cvalid) unsafeAtomicAdd(drow + (size_t)w * C, g);
      }
    }
  }
}

int ra_check(int R, int N, int C, int H, int W, int ph, int pw, float scale, int sampling) {
  if (R < 0 || N <= 0 || C <= 0 || H <= 0 || W <= 0 || ph <= 0 || pw <= 0) return NAWS_ERR_SHAPE;
  if (sampling < 0 || !(scale > 0.0f)) return NAWS_ERR_ARG;
  return NAWS_OK;
}

// dynamic LDS of a launch, 0 when it does not fit (the tables and the staging tiles)
size_t ra_lds_bytes(int ph, int pw, int H, int W, bool bwd) {
  const size_t nb = (size_t)ph * pw;
  if (nb > 160 * 1024 || (size_t)ph * H > 40 * 1024 || (size_t)pw * W > 40 * 1024) return 0;
  const size_t floats = ra_table_floats(ph, pw, H, W) +
                        RA_WAVES * (nb * RA_STRIDE + (bwd ? (size_t)pw * NAWS_WAVE : 0));
  return floats * sizeof(float) <= 160 * 1024 ? floats * sizeof(float) : 0;
}

}  // namespace

extern "C" int naws_roi_align_fwd(const float* X, int N, int C, int H, int W, const float* rois,
                                  int R, int pooled_h, int pooled_w, float spatial_scale,
                                  int sampling_ratio, float* Y, void* stream) {
  int rc = ra_check(R, N, C, H, W, pooled_h, pooled_w, spatial_scale, sampling_ratio);
  if (rc != NAWS_OK) return rc;
  if (R > 0) { NAWS_REQUIRE_PTR(X); NAWS_REQUIRE_PTR(rois); NAWS_REQUIRE_PTR(Y); }
  const size_t lds = ra_lds_bytes(pooled_h, pooled_w, H, W, false);
  if (lds == 0 || naws_cdiv(C, NAWS_WAVE * RA_WAVES) > 65535) return NAWS_ERR_UNSUPPORTED;
  if (R == 0) return NAWS_OK;
  if (lds > 64 * 1024 && naws_allow_lds(roi_align_fwd_kernel) != NAWS_OK) return NAWS_ERR_LAUNCH;
  dim3 grid((unsigned)R, (unsigned)naws_cdiv(C, NAWS_WAVE * RA_WAVES));
  hipLaunchKernelGGL(roi_align_fwd_kernel, grid, dim3(RA_TB), lds, (hipStream_t)stream, X, N, C, H, W,
                     rois, pooled_h, pooled_w, spatial_scale, sampling_ratio, Y);
  return naws_check_launch();
}

extern "C" int naws_roi_align_bwd(const float* dY, const float* rois, int R, int N, int C, int H,
                                  int W, int pooled_h, int pooled_w, float spatial_scale,
                                  int sampling_ratio, float* dX, void* stream) {
  int rc = ra_check(R, N, C, H, W, pooled_h, pooled_w, spatial_scale, sampling_ratio);
  if (rc != NAWS_OK) return rc;
  NAWS_REQUIRE_PTR(dX);
  if (R > 0) { NAWS_REQUIRE_PTR(dY); NAWS_REQUIRE_PTR(rois); }
  const size_t lds = ra_lds_bytes(pooled_h, pooled_w, H, W, true);
  if (lds == 0 || naws_cdiv(C, NAWS_WAVE * RA_WAVES) > 65535) return NAWS_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(dX, 0, (size_t)N * C * H * W * sizeof(float), s);
  if (e != hipSuccess) {
    g_naws_last_hip_error = (int)e;
    return NAWS_ERR_LAUNCH;
  }
  if (R == 0) return NAWS_OK;
  if (lds > 64 * 1024 && naws_allow_lds(roi_align_bwd_kernel) != NAWS_OK) return NAWS_ERR_LAUNCH;
  dim3 grid((unsigned)R, (unsigned)naws_cdiv(C, NAWS_WAVE * RA_WAVES));
  hipLaunchKernelGGL(roi_align_bwd_kernel, grid, dim3(RA_TB), lds, s, dY, rois, N, C, H, W, pooled_h,
                     pooled_w, spatial_scale, sampling_ratio, dX);
  return naws_check_launch();
}
