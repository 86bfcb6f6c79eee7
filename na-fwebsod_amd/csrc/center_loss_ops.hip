// WSL.CENTER_LOSS: the multi-centre feature loss of the WSDDN / noise-aware heads.
//   CenterLoss          ref: detectron/ops/center_loss_op.cu:33-278   (schema center_loss_op.cc:12-32)
//   CenterLossGradient  ref: detectron/ops/center_loss_op.cu:280-568  (schema center_loss_op.cc:34-69)
// The reference selects the top-k rois of every labelled class on the HOST (:102-174) and blocks
// after each of its C x M distance dots (:201-207), after the selector copy (:467-488), after the
// seed copy (:498-501) and after the count copy (:545-547): more than 100 synchronisations per
// iteration.  Here selection, centre choice, loss, both gradients and the centre update stay on the
// device: nothing below synchronises, allocates or copies to the host, and a sequence of the three
// entries can be captured in a graph.  oicr_ops.hip's conventions: wave64, TB = 256, first-index-
// wins argmax, every floating-point sum in a FIXED order (no float atomics), so results are
// reproducible run to run.
#include <float.h>
#include "naws_common.h"

namespace {

constexpr int TB = 256;

// (value, index) argmax with "first index wins ties" = the reference's strict '<' scan order.
struct Best {
  float v;
  int i;
};
__device__ __forceinline__ Best better(Best a, Best b) {
  if (b.i < 0) return a;
  if (a.i < 0) return b;
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}
__device__ __forceinline__ Best block_best(Best x, Best* sh) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    Best o;
    o.v = __shfl_xor(x.v, d);
    o.i = __shfl_xor(x.i, d);
    x = better(x, o);
  }
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = x;
  __syncthreads();
  Best r = sh[0];
  for (int k = 1; k < TB / 64; ++k) r = better(r, sh[k]);
  return r;
}

// fixed-order block sum (every thread gets the result)
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
  for (int k = 1; k < TB / 64; ++k) r += sh[k];
  return r;
}

// Workspace layout (int32 words; every section starts on a 16-byte boundary):
//   picks [c][top_k]  the selected rois in ascending index order, -1 rows for inactive classes
//   tmp   [c][top_k]  the same in selection order (the exclusion list while selecting)
//   act   [c]         1 active, 0 inactive, -1 active but fewer than top_k selectable rois
//   ngt   [4]         word 0: number of active classes (the reference's num_gt_class)
//   dots  [c][m]      fp32 squared distances
//   cdot  [c]         fp32 distance of the chosen centre
struct Ws {
  int* picks;
  int* tmp;
  int* act;
  int* ngt;
  float* dots;
  float* cdot;
};
static inline int64_t pad4(int64_t words) { return (words + 3) / 4 * 4; }
static inline int64_t ws_words(int c, int m, int top_k) {
  return 2 * pad4((int64_t)c * top_k) + pad4(c) + 4 + pad4((int64_t)c * m) + pad4(c);
}
static inline Ws ws_split(void* workspace, int c, int m, int top_k) {
  Ws w;
  int* p = (int*)workspace;
  w.picks = p; p += pad4((int64_t)c * top_k);
  w.tmp = p;   p += pad4((int64_t)c * top_k);
  w.act = p;   p += pad4(c);
  w.ngt = p;   p += 4;
  w.dots = (float*)p; p += pad4((int64_t)c * m);
  w.cdot = (float*)p;
  return w;
}

// ---- select: one block per class (center_loss_op.cu:121-174) -----------------------------------
__global__ __launch_bounds__(TB) void cl_select_kernel(const float* __restrict__ X,
                                                       const float* __restrict__ P, int n, int c,
                                                       int top_k, int ignore_label, int enabled,
                                                       int* __restrict__ picks, int* tmp,
                                                       int* __restrict__ act) {
  __shared__ Best sh[TB / 64];
  __shared__ int s_fail;
  const int cc = blockIdx.x;
  int* row = picks + (size_t)cc * top_k;
  int* sel = tmp + (size_t)cc * top_k;
  // block-uniform: the label test is '< 0.5 -> skip' (:142), so 0.5 itself and NaN are active
  const bool on = enabled && cc != ignore_label && n >= top_k && !(X[cc] < 0.5f);
  if (!on) {
    for (int k = threadIdx.x; k < top_k; k += TB) row[k] = -1;
    if (threadIdx.x == 0) act[cc] = 0;
    return;
  }
  if (threadIdx.x == 0) s_fail = 0;
  for (int k = 0; k < top_k; ++k) {
    Best b;
    b.v = -FLT_MAX; b.i = -1;
    for (int i = threadIdx.x; i < n; i += TB) {
      const float v = P[(size_t)i * c + cc];
      if (b.v < v) {                                  // strict: -FLT_MAX and NaN never win
        bool seen = false;
        for (int j = 0; j < k; ++j) seen |= (sel[j] == i);
        if (!seen) { b.v = v; b.i = i; }
      }
    }
    b = block_best(b, sh);
    if (threadIdx.x == 0) {
      sel[k] = b.i;
      if (b.i < 0) s_fail = 1;
    }
    __syncthreads();                                  // sel[k] is visible to the next round
  }
  if (s_fail) {                                       // the reference fails the net here (:161-166)
    for (int k = threadIdx.x; k < top_k; k += TB) row[k] = -1;
    if (threadIdx.x == 0) act[cc] = -1;
    return;
  }
  // std::set iteration order (:192): ascending roi index.  The picks are distinct: rank = position.
  for (int k = threadIdx.x; k < top_k; k += TB) {
    const int me = sel[k];
    int rank = 0;
    for (int j = 0; j < top_k; ++j) rank += (sel[j] < me) ? 1 : 0;
    row[rank] = me;
  }
  if (threadIdx.x == 0) act[cc] = 1;
}

// ---- distance: one block per (centre, class) over top_k x d (:189-207) -------------------------
__global__ __launch_bounds__(TB) void cl_dist_kernel(const float* __restrict__ F,
                                                     const float* __restrict__ CF, int m, int d,
                                                     int top_k, const int* __restrict__ picks,
                                                     const int* __restrict__ act,
                                                     float* __restrict__ dots) {
  __shared__ float sh[TB / 64];
  const int mm = blockIdx.x, cc = blockIdx.y;
  if (act[cc] != 1) {                                 // block-uniform
    if (threadIdx.x == 0) dots[(size_t)cc * m + mm] = 0.f;
    return;
  }
  const float* ctr = CF + ((size_t)cc * m + mm) * d;
  const int* row = picks + (size_t)cc * top_k;
  float acc = 0.f;
  // float4 loads need d % 4 == 0 AND 16-byte aligned bases (a caller may pass a row-offset pointer
  // into a flat buffer); anything else takes the scalar loop.  Block-uniform.
  const bool vec = (d & 3) == 0 && (((uintptr_t)F | (uintptr_t)CF) & 15) == 0;
  if (vec) {
    const int d4 = d >> 2;
    const int total = top_k * d4;
    for (int e = threadIdx.x; e < total; e += TB) {
      const int k = e / d4, q = e - k * d4;
      const float4 f = reinterpret_cast<const float4*>(F + (size_t)row[k] * d)[q];
      const float4 g = reinterpret_cast<const float4*>(ctr)[q];
      const float a0 = f.x - g.x, a1 = f.y - g.y, a2 = f.z - g.z, a3 = f.w - g.w;
      acc += a0 * a0; acc += a1 * a1; acc += a2 * a2; acc += a3 * a3;
    }
  } else {
    const int total = top_k * d;
    for (int e = threadIdx.x; e < total; e += TB) {
      const int k = e / d, q = e - k * d;
      const float a = F[(size_t)row[k] * d + q] - ctr[q];
      acc += a * a;
    }
  }
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) dots[(size_t)cc * m + mm] = acc;
}

// ---- centre choice: one block per class writes S, D, the class's distance (:186-221) -----------
__global__ __launch_bounds__(TB) void cl_choose_kernel(const float* __restrict__ F,
                                                       const float* __restrict__ CF, int m, int d,
                                                       int top_k, const int* __restrict__ picks,
                                                       const int* __restrict__ act,
                                                       const float* __restrict__ dots,
                                                       float* __restrict__ D, float* __restrict__ S,
                                                       float* __restrict__ cdot,
                                                       int32_t* __restrict__ counts) {
  const int cc = blockIdx.x;
  float* Dc = D + (size_t)cc * top_k * d;
  const size_t total = (size_t)top_k * d;
  int sel = -1;
  float best = FLT_MAX;
  if (act[cc] == 1)
    for (int mm = 0; mm < m; ++mm) {                  // strict '<' from FLT_MAX: first centre wins ties
      const float v = dots[(size_t)cc * m + mm];
      if (v < best) { best = v; sel = mm; }
    }
  if (threadIdx.x == 0) {
    S[cc] = (float)sel;
    cdot[cc] = best;
    if (counts && sel >= 0) counts[(size_t)cc * m + sel] += 1;
  }
  if (sel < 0) {
    for (size_t e = threadIdx.x; e < total; e += TB) Dc[e] = 0.f;
    return;
  }
  const float* ctr = CF + ((size_t)cc * m + sel) * d;
  const int* row = picks + (size_t)cc * top_k;
  for (size_t e = threadIdx.x; e < total; e += TB) {
    const int k = (int)(e / d), q = (int)(e - (size_t)k * d);
    Dc[e] = F[(size_t)row[k] * d + q] - ctr[q];
  }
}

// ---- loss: classes in ascending order, the reference's chain of float divisions (:221-227) ------
__global__ void cl_loss_kernel(const int* __restrict__ act, const float* __restrict__ cdot, int c,
                               int d, int top_k, int* __restrict__ ngt, float* __restrict__ L) {
  if (threadIdx.x != 0) return;
  float dot = 0.f;
  int num_gt = 0;
  bool fail = false;
  for (int cc = 0; cc < c; ++cc) {
    const int a = act[cc];
    if (a == 0) continue;
    ++num_gt;
    if (a < 0) fail = true; else dot += cdot[cc];
  }
  ngt[0] = num_gt;
  float loss = num_gt > 0 ? dot / num_gt / top_k / d / 2.f : 0.f;
  // the reference fails the net when a class runs out of rois (:161-166): poison the loss instead
  if (fail) loss = __int_as_float(0x7fc00000);
  L[0] = loss;
}

// ---- backward: feature gradient, one block per roi (:516-537) ----------------------------------
__global__ __launch_bounds__(TB) void cl_bwd_feat_kernel(const float* __restrict__ D,
                                                         const float* __restrict__ dL, int c, int d,
                                                         int top_k, int enabled,
                                                         const int* __restrict__ picks,
                                                         const int* __restrict__ ngt,
                                                         float* __restrict__ dF) {
  const int r = blockIdx.x;
  float* out = dF + (size_t)r * d;
  const int np = c * top_k;
  int hit = 0;
  if (enabled)
    for (int j = threadIdx.x; j < np; j += TB) hit |= (picks[j] == r);
  if (!__syncthreads_or(hit)) {
    for (int q = threadIdx.x; q < d; q += TB) out[q] = 0.f;
    return;
  }
  const int num_gt = ngt[0];
  // dL / num_gt / top_k / d (:503-504), rounded once instead of after every division
  const float alpha = num_gt > 0 ? (float)((double)dL[0] / num_gt / top_k / d) : 0.f;
  for (int q = threadIdx.x; q < d; q += TB) {
    float v = 0.f;
    for (int j = 0; j < np; ++j)                      // (class, k) ascending; the index is uniform
      if (picks[j] == r) v += alpha * D[(size_t)j * d + q];
    out[q] = v;
  }
}

// ---- backward: this iteration's centre contribution, one block per (centre, class) (:466-537) --
__global__ __launch_bounds__(TB) void cl_bwd_center_kernel(const float* __restrict__ D,
                                                           const float* __restrict__ S, int m, int d,
                                                           int top_k, float* __restrict__ dCF,
                                                           float* __restrict__ ndCF) {
  const int mm = blockIdx.x, cc = blockIdx.y;
  const bool mine = ((int)S[cc] == mm);               // S = -1 for inactive classes
  float* out = dCF + ((size_t)cc * m + mm) * d;
  if (threadIdx.x == 0) ndCF[(size_t)cc * m + mm] = mine ? 1.f : 0.f;
  const float* Dc = D + (size_t)cc * top_k * d;
  for (int q = threadIdx.x; q < d; q += TB) {
    float v = 0.f;
    if (mine)
      for (int k = 0; k < top_k; ++k) v -= Dc[(size_t)k * d + q];
    out[q] = v;
  }
}

// ---- state: accumulate the (all-reduced) previous contribution, update the centres (:340-379,
// :540-565).  One block per (class, centre) row. ------------------------------------------------
__global__ __launch_bounds__(TB) void cl_update_kernel(float* __restrict__ CF,
                                                       float* __restrict__ dCF,
                                                       float* __restrict__ ndCF,
                                                       float* __restrict__ acc_d,
                                                       float* __restrict__ acc_n, int d, int top_k,
                                                       float lr, int first, int apply) {
  const size_t rowi = blockIdx.x;
  float n_acc = first ? 0.f : acc_n[rowi] + ndCF[rowi];
  __syncthreads();                                    // every thread has read the row's count
  // lr * -1 / (int(count) * top_k + 1), :550-556
  const float coef = lr * -1.f / (float)((int)n_acc * top_k + 1);
  float* a = acc_d + rowi * d;
  float* g = dCF + rowi * d;
  float* w = CF + rowi * d;
  for (int q = threadIdx.x; q < d; q += TB) {
    float v = first ? 0.f : a[q] + g[q];
    if (first) g[q] = 0.f;
    if (apply) { w[q] = coef * v + w[q]; v = 0.f; }
    a[q] = v;
  }
  if (threadIdx.x == 0) {
    if (first) ndCF[rowi] = 0.f;
    acc_n[rowi] = apply ? 0.f : n_acc;
  }
}

}  // namespace

extern "C" int64_t naws_center_loss_workspace_bytes(int c, int m, int top_k) {
  if (c <= 0 || m <= 0 || top_k <= 0) return 0;
  return ws_words(c, m, top_k) * 4;
}

extern "C" int naws_center_loss_fwd(const float* X, const float* P, const float* F, const float* CF,
                                    int n, int c, int m, int d, int top_k, int ignore_label,
                                    int enabled, void* workspace, float* L, float* D, float* S,
                                    int32_t* counts, void* stream) {
  if (n < 0 || c <= 0 || m <= 0 || d <= 0 || top_k <= 0) return NAWS_ERR_SHAPE;
  NAWS_REQUIRE_PTR(X); NAWS_REQUIRE_PTR(CF); NAWS_REQUIRE_PTR(workspace);
  NAWS_REQUIRE_PTR(L); NAWS_REQUIRE_PTR(D); NAWS_REQUIRE_PTR(S);
  if (n > 0) { NAWS_REQUIRE_PTR(P); NAWS_REQUIRE_PTR(F); }
  hipStream_t s = (hipStream_t)stream;
  const Ws w = ws_split(workspace, c, m, top_k);
  hipLaunchKernelGGL(cl_select_kernel, dim3(c), dim3(TB), 0, s, X, P, n, c, top_k, ignore_label,
                     enabled ? 1 : 0, w.picks, w.tmp, w.act);
  hipLaunchKernelGGL(cl_dist_kernel, dim3(m, c), dim3(TB), 0, s, F, CF, m, d, top_k, w.picks, w.act,
                     w.dots);
  hipLaunchKernelGGL(cl_choose_kernel, dim3(c), dim3(TB), 0, s, F, CF, m, d, top_k, w.picks, w.act,
                     w.dots, D, S, w.cdot, counts);
  hipLaunchKernelGGL(cl_loss_kernel, dim3(1), dim3(64), 0, s, w.act, w.cdot, c, d, top_k, w.ngt, L);
  return naws_check_launch();
}

extern "C" int naws_center_loss_bwd(const float* D, const float* S, const float* dL, int n, int c,
                                    int m, int d, int top_k, int enabled, const void* workspace,
                                    float* dF, float* dCF, float* ndCF, void* stream) {
  if (n < 0 || c <= 0 || m <= 0 || d <= 0 || top_k <= 0) return NAWS_ERR_SHAPE;
  NAWS_REQUIRE_PTR(D); NAWS_REQUIRE_PTR(S); NAWS_REQUIRE_PTR(dL); NAWS_REQUIRE_PTR(workspace);
  NAWS_REQUIRE_PTR(dCF); NAWS_REQUIRE_PTR(ndCF);
  if (n > 0) NAWS_REQUIRE_PTR(dF);
  hipStream_t s = (hipStream_t)stream;
  const Ws w = ws_split(const_cast<void*>(workspace), c, m, top_k);
  if (n > 0)
    hipLaunchKernelGGL(cl_bwd_feat_kernel, dim3(n), dim3(TB), 0, s, D, dL, c, d, top_k,
                       enabled ? 1 : 0, w.picks, w.ngt, dF);
  if (enabled)                                        // past max_iter the in-place blobs stay (:329-331)
    hipLaunchKernelGGL(cl_bwd_center_kernel, dim3(m, c), dim3(TB), 0, s, D, S, m, d, top_k, dCF,
                       ndCF);
  return naws_check_launch();
}

extern "C" int naws_center_loss_update(float* CF, float* dCF, float* ndCF, float* acc_dCF,
                                       float* acc_ndCF, int c, int m, int d, int top_k, float lr,
                                       int first, int apply, void* stream) {
  if (c <= 0 || m <= 0 || d <= 0 || top_k <= 0) return NAWS_ERR_SHAPE;
  NAWS_REQUIRE_PTR(CF); NAWS_REQUIRE_PTR(dCF); NAWS_REQUIRE_PTR(ndCF);
  NAWS_REQUIRE_PTR(acc_dCF); NAWS_REQUIRE_PTR(acc_ndCF);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cl_update_kernel, dim3((unsigned)((int64_t)c * m)), dim3(TB), 0, s, CF, dCF,
                     ndCF, acc_dCF, acc_ndCF, d, top_k, lr, first ? 1 : 0, apply ? 1 : 0);
  return naws_check_launch();
}
