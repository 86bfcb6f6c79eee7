// Box-proposal recall: the greedy one-to-one matching of proposals to ground truth.
//   evaluate_box_proposals  ref: detectron/datasets/json_dataset_evaluator.py:255-336 (loop :305-321)
//   bbox_overlaps           ref: detectron/utils/cython_bbox.pyx:27-63
// The reference builds a dense [P, G] overlap matrix per image and per (area range, limit) setting
// and runs min(P, G) rounds of argmax / max / mark-with--1 over it in Python.  An image under one
// setting is independent of every other, so: one wave per (image, setting), grid-stride over
// images x settings, lanes over the image's proposals, the image's ground truth in LDS.
//
// Which of the two forms this is: the CACHED one.  Every valid gt keeps its best unused proposal
// (overlap, proposal index) in one 64-bit key; a round takes the best key over the gt, and only
// the gt whose cached proposal was just consumed are computed again.  An image costs about G * P
// overlaps plus G * G / 64 key reads, not the G * G * P of recomputing every column every round -
// with 2000 proposals and a few dozen gt that is the difference between 40 and 1600 passes over
// the proposals.  (All gt sharing one best proposal - identical boxes - is the worst case and
// falls back to G * G * P; it stays correct.)
//
// Keys.  An overlap here is >= 0, so its float bits order like an unsigned word.  Per gt:
// bits(overlap) << 32 | ~proposal: the maximum is the greatest overlap and, among equals, the
// LOWEST proposal index = the first maximum of the column argmax (a used row holds -1 there and
// never wins while an unused one exists).  Across gt: bits(overlap) << 32 | ~gt: the first
// maximum of max_overlaps.argmax().  Key 0 = no candidate (gt outside the area range, already
// matched, or no unused proposal left).
//
// State.  The per-gt keys and the used-proposal bits live in a per-wave slot of the caller's
// workspace, and every word of either has ONE lane that reads and writes it (gt g: lane g % 64;
// proposal p = lane + 64 k: bit k % 32 of word (k / 32) * 64 + lane), so no value crosses lanes
// through memory; what crosses goes through shuffles.  No atomics; one writer per output element.
// Every overlap operation is ONE IEEE operation (contraction off for the whole file).
#pragma clang fp contract(off)
#include <limits.h>
#include "naws_common.h"

namespace {

constexpr int TB = 256;                 // 4 waves
constexpr int WAVES = TB / NAWS_WAVE;
constexpr int MATCH_MAX_BLOCKS = 1024;  // grid cap: 4096 waves stride over images x settings
constexpr int GCAP = 256;               // gt boxes of a segment held in LDS (more: read from memory)
constexpr int MAX_SET = 64;             // area ranges / limits per launch (each)

struct MatchSettings {
  float lo[MAX_SET], hi[MAX_SET];
  int32_t limit[MAX_SET];
};

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t u = __shfl_xor((unsigned long long)v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

// cython_bbox.pyx:44-47 box_area of a query box: float differences, `+ 1` and the product in
// double, stored as float
__device__ __forceinline__ float query_area(const float4 q) {
  return (float)(((double)(q.z - q.x) + 1.0) * ((double)(q.w - q.y) + 1.0));
}

// cython_bbox.pyx:48-62
__device__ __forceinline__ float overlap(const float4 b, const float4 q, const float qa) {
  const float iw = (float)((double)(fminf(b.z, q.z) - fmaxf(b.x, q.x)) + 1.0);
  const float ih = (float)((double)(fminf(b.w, q.w) - fmaxf(b.y, q.y)) + 1.0);
  if (!(iw > 0.f && ih > 0.f)) return 0.f;
  const float inter = iw * ih;
  const double barea = ((double)(b.z - b.x) + 1.0) * ((double)(b.w - b.y) + 1.0);
  const float ua = (float)(barea + (double)qa - (double)inter);
  return __fdiv_rn(inter, ua);
}

// the best unused proposal of one gt box: wave-uniform result
__device__ __forceinline__ uint64_t best_proposal(const float4* __restrict__ boxes, int64_t p0,
                                                  int64_t np, const float4 q, const uint32_t* bits,
                                                  int lane) {
  const float qa = query_area(q);
  uint64_t best = 0;
  uint32_t word = 0;
  int64_t k = 0;
  for (int64_t p = lane; p < np; p += 64, ++k) {
    if ((k & 31) == 0) word = bits[(k >> 5) * 64 + lane];
    if ((word >> (k & 31)) & 1u) continue;
    const float v = overlap(boxes[p0 + p], q, qa);
    const uint64_t key = ((uint64_t)__float_as_uint(v) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)p);
    best = key > best ? key : best;
  }
  return wave_max_u64(best);
}

__global__ __launch_bounds__(TB) void proposal_match_kernel(
    const float4* __restrict__ boxes, const int64_t* __restrict__ box_off, int64_t Pt,
    const float4* __restrict__ gt, const float* __restrict__ gt_area,
    const int64_t* __restrict__ gt_off, int64_t Gt, int64_t S, MatchSettings st, int A, int L,
    int64_t max_props, int64_t max_gt, char* workspace, int64_t slot_bytes, float* gt_iou) {
  __shared__ float4 sh_gt[WAVES][GCAP];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t wave0 = (int64_t)blockIdx.x * WAVES + wv;
  const int64_t nwaves = (int64_t)gridDim.x * WAVES;
  uint64_t* keys = (uint64_t*)(workspace + wave0 * slot_bytes);      // [max_gt]
  uint32_t* bits = (uint32_t*)(keys + max_gt);                       // [cdiv(max_props, 2048) * 64]
  const int64_t nset = (int64_t)A * L, items = S * nset;
  for (int64_t item = wave0; item < items; item += nwaves) {         // wave-uniform
    const int64_t s = item / nset, q = item - s * nset;
    const int a = (int)(q / L), l = (int)(q - (int64_t)a * L);
    const int64_t p0 = box_off[s], p1 = box_off[s + 1];
    const int64_t g0 = gt_off[s], g1 = gt_off[s + 1];
    // the offsets live on the device, so the entry cannot check them: a segment that leaves its
    // arrays or the workspace touches nothing
    if (p0 < 0 || p1 < p0 || p1 > Pt || g0 < 0 || g1 < g0 || g1 > Gt || p1 - p0 > max_props ||
        g1 - g0 > max_gt)
      continue;
    const int64_t P = p1 - p0, G = g1 - g0;
    const int64_t lim = st.limit[l];
    const int64_t np = (lim <= 0 || P < lim) ? P : lim;              // boxes[:limit]
    const float lo = st.lo[a], hi = st.hi[a];
    const bool in_lds = G <= GCAP;
    float* out = gt_iou + q * Gt + g0;
    const float4* sgt = gt + g0;
    const float* sarea = gt_area + g0;

    // validity, the outputs' first values, the gt boxes into LDS
    int64_t nvalid = 0;
    for (int64_t gb = 0; gb < G; gb += 64) {
      const int64_t g = gb + lane;
      bool v = false;
      if (g < G) {
        const float ar = sarea[g];
        v = lo <= ar && ar <= hi;
        out[g] = v ? (np == 0 ? -2.f : 0.f) : -1.f;
        keys[g] = 0;
        if (in_lds) sh_gt[wv][g] = sgt[g];
      }
      nvalid += __popcll(__ballot(v));
    }
    if (np == 0 || nvalid == 0) continue;
    for (int64_t i = lane; i < (np + 2047) / 2048 * 64; i += 64) bits[i] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");           // sh_gt is read across lanes
    __builtin_amdgcn_wave_barrier();

    // every valid gt's best proposal
    for (int64_t g = 0; g < G; ++g) {
      const float ar = sarea[g];                                     // wave-uniform
      if (!(lo <= ar && ar <= hi)) continue;
      const float4 qb = in_lds ? sh_gt[wv][g] : sgt[g];
      const uint64_t k = best_proposal(boxes, p0, np, qb, bits, lane);
      if (lane == (int)(g & 63)) keys[g] = k;
    }

    // the rounds
    const int64_t rounds = np < nvalid ? np : nvalid;
    for (int64_t j = 0; j < rounds; ++j) {
      uint64_t best = 0;
      for (int64_t g = lane; g < G; g += 64) {
        const uint64_t k = keys[g];
        if (k != 0) {
          const uint64_t k2 = (k & 0xFFFFFFFF00000000ull) | (uint64_t)(0xFFFFFFFFu - (uint32_t)g);
          best = k2 > best ? k2 : best;
        }
      }
      best = wave_max_u64(best);
      // overlap 0 at the top: every pair still unused is 0, and so is every remaining round's
      // record - the value those gt already hold
      if ((best >> 32) == 0) break;
      const uint32_t gs = 0xFFFFFFFFu - (uint32_t)best;
      const int owner = (int)(gs & 63);
      uint32_t bsel = 0;
      if (lane == owner) {
        bsel = 0xFFFFFFFFu - (uint32_t)keys[gs];
        out[gs] = __uint_as_float((uint32_t)(best >> 32));
        keys[gs] = 0;                                                // the gt is used
      }
      bsel = __shfl(bsel, owner, 64);
      if (lane == (int)(bsel & 63)) {                                // the proposal is used
        const uint32_t kk = bsel >> 6;
        bits[(int64_t)(kk >> 5) * 64 + lane] |= 1u << (kk & 31);
      }
      if (j + 1 == rounds) break;
      // only the gt that had cached this proposal look again
      for (int64_t gb = 0; gb < G; gb += 64) {
        const int64_t g = gb + lane;
        bool need = false;
        if (g < G) {
          const uint64_t k = keys[g];
          need = k != 0 && (uint32_t)k == 0xFFFFFFFFu - bsel;
        }
        unsigned long long mask = __ballot(need);
        const int n = __popcll(mask);
        for (int i = 0; i < n; ++i) {
          const int bit = __ffsll((long long)mask) - 1;
          mask &= mask - 1;
          const int64_t gg = gb + bit;
          const float4 qb = in_lds ? sh_gt[wv][gg] : sgt[gg];
          const uint64_t k = best_proposal(boxes, p0, np, qb, bits, lane);
          if (lane == bit) keys[gg] = k;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();                                 // sh_gt is rewritten next item
  }
}

int64_t slot_bytes_of(int64_t max_props, int64_t max_gt) {
  return (max_gt * 8 + naws_cdiv(max_props, 2048) * 64 * 4 + 15) / 16 * 16;
}

}  // namespace

extern "C" int naws_proposal_match_max_grid(void) { return MATCH_MAX_BLOCKS; }

extern "C" int64_t naws_proposal_match_workspace_bytes(int64_t max_props, int64_t max_gt) {
  if (max_props < 0 || max_gt < 0 || max_props > INT_MAX || max_gt > INT_MAX) return -1;
  return std::max<int64_t>(16, slot_bytes_of(max_props, max_gt) * MATCH_MAX_BLOCKS * WAVES);
}

extern "C" int naws_proposal_match_fwd(const float* boxes, const int64_t* box_off, int64_t P_total,
                                       const float* gt, const float* gt_area, const int64_t* gt_off,
                                       int64_t G_total, int64_t S, const float* area_lo,
                                       const float* area_hi, int num_areas, const int32_t* limits,
                                       int num_limits, int64_t max_props, int64_t max_gt,
                                       void* workspace, int64_t workspace_bytes, float* gt_iou,
                                       void* stream) {
  if (P_total < 0 || G_total < 0 || S < 0 || max_props < 0 || max_gt < 0 || workspace_bytes < 0)
    return NAWS_ERR_SHAPE;
  if (num_areas < 1 || num_limits < 1 || ((uintptr_t)boxes & 15) != 0 || ((uintptr_t)gt & 15) != 0 ||
      ((uintptr_t)workspace & 15) != 0)
    return NAWS_ERR_ARG;
  NAWS_REQUIRE_PTR(area_lo); NAWS_REQUIRE_PTR(area_hi); NAWS_REQUIRE_PTR(limits);
  NAWS_REQUIRE_PTR(box_off); NAWS_REQUIRE_PTR(gt_off); NAWS_REQUIRE_PTR(workspace);
  if (P_total > 0) NAWS_REQUIRE_PTR(boxes);
  if (G_total > 0) { NAWS_REQUIRE_PTR(gt); NAWS_REQUIRE_PTR(gt_area); NAWS_REQUIRE_PTR(gt_iou); }
  if (num_areas > MAX_SET || num_limits > MAX_SET || P_total > INT_MAX || G_total > INT_MAX ||
      S > INT_MAX / (MAX_SET * MAX_SET) || max_props > INT_MAX || max_gt > INT_MAX)
    return NAWS_ERR_UNSUPPORTED;
  for (int a = 0; a < num_areas; ++a)                    // host values, readable only now
    if (area_lo[a] != area_lo[a] || area_hi[a] != area_hi[a]) return NAWS_ERR_ARG;
  if (workspace_bytes < naws_proposal_match_workspace_bytes(max_props, max_gt)) return NAWS_ERR_SHAPE;
  if (S == 0 || G_total == 0) return NAWS_OK;
  MatchSettings st;
  for (int a = 0; a < MAX_SET; ++a) {
    st.lo[a] = a < num_areas ? area_lo[a] : 0.f;
    st.hi[a] = a < num_areas ? area_hi[a] : 0.f;
    st.limit[a] = a < num_limits ? limits[a] : 0;
  }
  const int64_t items = S * num_areas * num_limits;
  const int64_t blocks = std::min<int64_t>(naws_cdiv(items, WAVES), MATCH_MAX_BLOCKS);
  hipLaunchKernelGGL(proposal_match_kernel, dim3((unsigned)blocks), dim3(TB), 0, (hipStream_t)stream,
                     (const float4*)boxes, box_off, P_total, (const float4*)gt, gt_area, gt_off,
                     G_total, S, st, num_areas, num_limits, max_props, max_gt, (char*)workspace,
                     slot_bytes_of(max_props, max_gt), gt_iou);
  return naws_check_launch();
}
