// Test-time grid search over TEST.NMS x TEST.SCORE_THRESH x TEST.DETECTIONS_PER_IM (the sweep of
// the reference's tools/test_net_wsl_grid_search.py :157-187, which re-runs
// box_results_with_nms_and_limit, core/test_wsl.py:803-863, once per setting).
//   nms_multi   greedy NMS (utils/cython_nms.pyx:36-87) of every (image, class) list of a dataset
//               at up to 32 thresholds in ONE pass: whether a box is kept depends only on the boxes
//               visited before it, so a T-bit "suppressed" word per box is carried down the list and
//               every IoU is computed once for all thresholds.
//   grid_cut    the counts and the L-th surviving scores the image-wide DETECTIONS_PER_IM cut
//               (:849-863) needs, for every (image, NMS threshold): a segmented scan over one bit.
// The IoU is the expression of nms_ops.hip (nms_suppresses) operation for operation: fp32, each
// operation rounded on its own, so contraction is off for this whole file; an IoU that lands
// exactly on a threshold falls the same way in both.
#pragma clang fp contract(off)
#include <limits.h>
#include <math.h>
#include "naws_common.h"

namespace {

constexpr int TB = 256;                  // 4 waves
constexpr int WAVES = TB / NAWS_WAVE;
constexpr int NMS_LDS_BOXES = 2048;      // a longer list reads its boxes and words from memory
constexpr int NMS_MAX_LIST = 16384;      // the limit of naws_nms_sorted_fwd
constexpr int NMS_MAX_BLOCKS = 65535;    // grid cap: the workgroups stride over the lists
constexpr int CUT_MAX_BLOCKS = 16384;    // grid cap: the waves stride over the (image, t) pairs
constexpr int MAX_T = 32, MAX_S = 64, MAX_L = 64;

struct NmsThr { float v[MAX_T]; };
struct CutArgs {
  float s[MAX_S];
  int l[MAX_L];
};

__device__ __forceinline__ float nms_iou(const float4 a, const float4 b) {
  const float aw = a.z - a.x + 1.f, ah = a.w - a.y + 1.f;
  const float bw = b.z - b.x + 1.f, bh = b.w - b.y + 1.f;
  const float aa = aw * ah, ab = bw * bh;
  const float xx1 = a.x >= b.x ? a.x : b.x, yy1 = a.y >= b.y ? a.y : b.y;
  const float xx2 = a.z <= b.z ? a.z : b.z, yy2 = a.w <= b.w ? a.w : b.w;
  float w = xx2 - xx1 + 1.f, h = yy2 - yy1 + 1.f;
  w = 0.f >= w ? 0.f : w;
  h = 0.f >= h ? 0.f : h;
  const float inter = w * h;
  const float sum = aa + ab;
  const float uni = sum - inter;
  return inter / uni;
}

// The walk over one list.  bx / sp are the list's boxes and its "suppressed" words (all zero on
// entry), in LDS or in memory.  Every thread reads sp[i] (one address: a broadcast); a box that is
// dead at every threshold suppresses nothing and costs no barrier.  The barrier at the end of a
// live box's round orders its writes (sp[j], j > i) before the next reads of them: between two
// barriers no thread reads a word that another one writes.
template <typename BoxPtr, typename WordPtr>
__device__ __forceinline__ void nms_multi_walk(BoxPtr bx, WordPtr sp, int n, const NmsThr& thr, int T,
                                               uint32_t tmask) {
  for (int i = 0; i < n; ++i) {
    const uint32_t alive = ~sp[i] & tmask;               // block-uniform
    if (alive == 0u) continue;
    const float4 bi = bx[i];
    for (int j = i + 1 + (int)threadIdx.x; j < n; j += TB) {
      const uint32_t s = sp[j];
      if ((~s & alive) == 0u) continue;                  // nothing left that box i could suppress
      const float ovr = nms_iou(bi, bx[j]);
      uint32_t m = 0u;
#pragma unroll
      for (int t = 0; t < MAX_T; ++t)
        if (t < T && ovr >= thr.v[t]) m |= 1u << t;       // false for a NaN overlap, as in numpy
      sp[j] = s | (m & alive);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(TB) void nms_multi_kernel(const float4* __restrict__ boxes,
                                                       const int64_t* __restrict__ list_off,
                                                       int64_t total, int64_t nlists, NmsThr thr, int T,
                                                       uint32_t* surv, int32_t* __restrict__ status) {
  __shared__ float4 sh_box[NMS_LDS_BOXES];
  __shared__ uint32_t sh_sup[NMS_LDS_BOXES];
  const uint32_t tmask = T >= 32 ? 0xffffffffu : ((1u << T) - 1u);
  const int tid = threadIdx.x;
  for (int64_t li = blockIdx.x; li < nlists; li += gridDim.x) {     // block-uniform
    const int64_t o0 = list_off[li], o1 = list_off[li + 1];
    // the offsets live on the device, so the entry cannot check them: a list that leaves the
    // arrays, or is longer than the entry takes, is reported and touches nothing
    if (o0 < 0 || o1 < o0 || o1 > total) {
      if (tid == 0) status[li] = -2;
      continue;
    }
    if (o1 - o0 > NMS_MAX_LIST) {
      if (tid == 0) status[li] = -3;
      continue;
    }
    const int n = (int)(o1 - o0);
    const float4* bx = boxes + o0;
    uint32_t* out = surv + o0;
    if (n <= NMS_LDS_BOXES) {
      __syncthreads();                                   // the previous list's LDS image is done with
      for (int p = tid; p < n; p += TB) { sh_box[p] = bx[p]; sh_sup[p] = 0u; }
      __syncthreads();
      nms_multi_walk(sh_box, sh_sup, n, thr, T, tmask);
      for (int p = tid; p < n; p += TB) out[p] = ~sh_sup[p] & tmask;
    } else {
      // the output words are the working state; a workgroup's own writes are visible to it
      // behind its barrier
      for (int p = tid; p < n; p += TB) out[p] = 0u;
      __syncthreads();
      nms_multi_walk(bx, out, n, thr, T, tmask);
      for (int p = tid; p < n; p += TB) out[p] = ~out[p] & tmask;   // each thread its own words
    }
    if (tid == 0) status[li] = 0;
  }
}

// One wave per (image, NMS threshold) pair, lanes over 64 consecutive candidates of the image's
// descending-score list.  Lane s keeps count s and lane l keeps the score of limit l, so S and Lc
// are loops over wave-uniform values and nothing is indexed by a lane.
__global__ __launch_bounds__(TB) void grid_cut_kernel(const uint32_t* __restrict__ surv,
                                                      const float* __restrict__ score,
                                                      const int64_t* __restrict__ img_off, int64_t N,
                                                      int64_t I, int T, CutArgs a, int S, int Lc,
                                                      int32_t* __restrict__ count,
                                                      float* __restrict__ kth,
                                                      int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * WAVES;
  const unsigned long long le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);   // lanes <= mine
  for (int64_t w = wave0; w < I * T; w += nwaves) {      // wave-uniform
    const int64_t img = w / T;
    const int t = (int)(w - img * T);
    const int64_t o0 = img_off[img], o1 = img_off[img + 1];
    if (o0 < 0 || o1 < o0 || o1 > N) {                   // see nms_multi_kernel
      if (t == 0 && lane == 0) status[img] = -2;
      continue;
    }
    int mycnt = 0;
    float mykth = -INFINITY;                             // fewer than L survivors, or L <= 0
    long long running = 0;                               // survivors in front of this chunk
    for (int64_t base = o0; base < o1; base += 64) {
      const int64_t p = base + lane;
      const bool in = p < o1;
      const float sc = in ? score[p] : 0.f;
      const bool bit = in && ((surv[p] >> t) & 1u);
      const unsigned long long mask = __ballot(bit);
      if (mask == 0ull) continue;
      const int tot = __popcll(mask);
      for (int s = 0; s < S; ++s) {
        const int c = __popcll(__ballot(bit && sc > a.s[s]));
        if (lane == s) mycnt += c;
      }
      const int incl = __popcll(mask & le);               // survivors up to and including my lane
      for (int l = 0; l < Lc; ++l) {
        const long long L = a.l[l];
        if (L > running && L <= running + tot) {          // the L-th survivor sits in this chunk
          const unsigned long long hit = __ballot(bit && incl == (int)(L - running));
          const float v = __shfl(sc, __ffsll((long long)hit) - 1, 64);
          if (lane == l) mykth = v;
        }
      }
      running += tot;
    }
    const int64_t row = img * T + t;
    if (lane < S) count[row * S + lane] = mycnt;
    if (lane < Lc) kth[row * Lc + lane] = mykth;
    if (t == 0 && lane == 0) status[img] = 0;
  }
}

}  // namespace

extern "C" int naws_nms_multi_fwd(const float* boxes, const int64_t* list_off, int64_t total,
                                  int64_t nlists, const float* thresholds, int T, uint32_t* survive,
                                  int32_t* status, void* stream) {
  if (total < 0 || nlists < 0) return NAWS_ERR_SHAPE;
  if (T < 1 || ((uintptr_t)boxes & 15) != 0) return NAWS_ERR_ARG;
  NAWS_REQUIRE_PTR(thresholds); NAWS_REQUIRE_PTR(list_off);
  if (total > 0) { NAWS_REQUIRE_PTR(boxes); NAWS_REQUIRE_PTR(survive); }
  if (nlists > 0) NAWS_REQUIRE_PTR(status);
  if (T > MAX_T || total > INT_MAX || nlists > INT_MAX) return NAWS_ERR_UNSUPPORTED;
  for (int t = 0; t < T; ++t)                            // host values, readable only now
    if (thresholds[t] != thresholds[t]) return NAWS_ERR_ARG;
  if (nlists == 0) return NAWS_OK;
  NmsThr thr;
  for (int t = 0; t < MAX_T; ++t) thr.v[t] = t < T ? thresholds[t] : INFINITY;
  const int64_t blocks = std::min<int64_t>(nlists, NMS_MAX_BLOCKS);
  hipLaunchKernelGGL(nms_multi_kernel, dim3((unsigned)blocks), dim3(TB), 0, (hipStream_t)stream,
                     (const float4*)boxes, list_off, total, nlists, thr, T, survive, status);
  return naws_check_launch();
}

extern "C" int naws_grid_cut_fwd(const uint32_t* survive, const float* score, const int64_t* img_off,
                                 int64_t N, int64_t I, int T, const float* score_thresholds, int S,
                                 const int32_t* limits, int Lc, int32_t* count, float* kth,
                                 int32_t* status, void* stream) {
  if (N < 0 || I < 0 || S < 0 || Lc < 0) return NAWS_ERR_SHAPE;
  if (T < 1) return NAWS_ERR_ARG;
  if (S > 0) NAWS_REQUIRE_PTR(score_thresholds);
  if (Lc > 0) NAWS_REQUIRE_PTR(limits);
  NAWS_REQUIRE_PTR(img_off);
  if (N > 0) { NAWS_REQUIRE_PTR(survive); NAWS_REQUIRE_PTR(score); }
  if (I > 0) {
    NAWS_REQUIRE_PTR(status);
    if (S > 0) NAWS_REQUIRE_PTR(count);
    if (Lc > 0) NAWS_REQUIRE_PTR(kth);
  }
  if (T > MAX_T || S > MAX_S || Lc > MAX_L || N > INT_MAX || I > INT_MAX / MAX_T)
    return NAWS_ERR_UNSUPPORTED;
  for (int s = 0; s < S; ++s)                            // host values, readable only now
    if (score_thresholds[s] != score_thresholds[s]) return NAWS_ERR_ARG;
  if (I == 0) return NAWS_OK;
  CutArgs a;
  for (int s = 0; s < MAX_S; ++s) a.s[s] = s < S ? score_thresholds[s] : INFINITY;
  for (int l = 0; l < MAX_L; ++l) a.l[l] = l < Lc ? limits[l] : 0;
  const int64_t blocks = std::min<int64_t>(naws_cdiv(I * T, WAVES), CUT_MAX_BLOCKS);
  hipLaunchKernelGGL(grid_cut_kernel, dim3((unsigned)blocks), dim3(TB), 0, (hipStream_t)stream,
                     survive, score, img_off, N, I, T, a, S, Lc, count, kth, status);
  return naws_check_launch();
}
