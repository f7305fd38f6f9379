// mpe_rig_peel.hip — the step between the rounds of mpe_rig_init_bodies_batch (mpe_rig.cpp): several bodies found in one
// frame, body after body, each in the detections the earlier ones left.  The logic is mpe_rig_peel.h (shared with the CPU
// tier); the rounds themselves are launch_k_rig_init (mpe_k3.hip), unchanged, over the lists this step writes.
//
// Three launches on one stream in front of round b, kernel boundaries order them:
//   k_rig_peel_count    a wave per (problem, camera) list, lane j owns detection j: the owner byte, with the claims of
//                       round b - 1 folded in; that round's answer translated to the caller's indices and written to the
//                       call's records; a __ballot of "free for body b" and its popcount -> the list's count
//   k_rig_peel_scan     one block: the exclusive scan of the counts -> the round's det_begin.  k_rig_init_* address the
//                       lists of problem i as det_begin + i * n_cam and read n_cam + 1 entries, so the compacted lists are
//                       contiguous across the whole call
//   k_rig_peel_scatter  a wave per list again: the popcount of the lower free lanes is the order-preserving position;
//                       coordinates and index map (compacted -> caller's) to that position
// Behind the last round k_rig_peel_count runs once more, alone: the last claims and the last translation.
// No atomics, no early return of part of a wave in front of a ballot or a barrier, plain vector stores only.
#include "mpe_internal.h"
#include "mpe_rig_peel.h"

namespace mpe {
namespace {

__global__ __launch_bounds__(MPE_RIG_PEEL_LANES) void k_rig_peel_count(RigPeelDev d, int round, int n_mk_prev) {
  static_assert(MPE_RIG_PEEL_LANES == 64 && MPE_MAX_DETECTIONS <= MPE_RIG_PEEL_LANES, "one lane per detection of a list");
  const int list = (int)blockIdx.x, j = (int)threadIdx.x;  // (the grid is the lists: block-uniform from here)
  const int i = list / d.n_cam, c = list - i * d.n_cam;
  const int b0 = d.det_begin[list];
  const int n = min(d.det_begin[list + 1] - b0, MPE_MAX_DETECTIONS);
  int8_t own = MPE_RIG_PEEL_TAKEN;
  if (j < n) own = round == 0 ? d.owner_in[b0 + j] : d.owner[b0 + j];
  if (round > 0) {
    const int pb = round - 1;
    const size_t rec = (size_t)i * d.n_bodies + pb;
    const bool asked = d.find[rec] != 0;
    const int* map = d.map + d.r_begin[list];
    const uint32_t* words = d.r_match + (size_t)list * n_mk_prev;
    if (asked) own = rig_peel_fold(own, j, d.r_info[i].reason == 0, words, n_mk_prev, map, pb);
    if (j < MPE_MAX_MARKERS)
      d.match[(rec * d.n_cam + c) * MPE_MAX_MARKERS + j] = (asked && j < n_mk_prev) ? rig_peel_word(words[j], map) : 0u;
    if (c == 0 && j == 0) {  // the record and the info of (i, pb): one lane, two struct copies
      if (asked) {
        const int cam = d.r_info[i].camera;
        d.out[rec] = d.r_out[i];
        rig_peel_info(d.r_info[i], cam >= 0 ? d.map + d.r_begin[(size_t)i * d.n_cam + cam] : nullptr, &d.info[rec]);
      } else {
        rig_peel_not_asked(&d.out[rec], &d.info[rec]);
      }
    }
  }
  if (j < n) d.owner[b0 + j] = own;
  const bool more = round < d.n_bodies;  // (uniform)
  const bool free_now = more && j < n && own == MPE_RIG_PEEL_FREE && d.find[(size_t)i * d.n_bodies + round] != 0;
  const unsigned long long mask = __ballot(free_now);
  if (more && j == 0) d.counts[list] = rig_peel_count(mask);
}

// counts (n) -> begin (n + 1), exclusive; one block, every lane a run of consecutive lists
__global__ __launch_bounds__(MPE_RIG_PEEL_SCAN_LANES) void k_rig_peel_scan(const int* __restrict__ counts, int n,
                                                                         int* __restrict__ begin) {
  __shared__ int s_sum[MPE_RIG_PEEL_SCAN_LANES];
  const int t = (int)threadIdx.x;
  const int run = (n + MPE_RIG_PEEL_SCAN_LANES - 1) / MPE_RIG_PEEL_SCAN_LANES;
  const int lo = min(t * run, n), hi = min(lo + run, n);
  int sum = 0;
  for (int k = lo; k < hi; ++k) sum += counts[k];
  s_sum[t] = sum;
  __syncthreads();
  int base = 0;
  for (int k = 0; k < t; ++k) base += s_sum[k];
  for (int k = lo; k < hi; ++k) {
    begin[k] = base;
    base += counts[k];
  }
  if (t == MPE_RIG_PEEL_SCAN_LANES - 1) begin[n] = base;
}

__global__ __launch_bounds__(MPE_RIG_PEEL_LANES) void k_rig_peel_scatter(RigPeelDev d, int round) {
  const int list = (int)blockIdx.x, j = (int)threadIdx.x;
  const int i = list / d.n_cam;
  const int b0 = d.det_begin[list];
  const int n = min(d.det_begin[list + 1] - b0, MPE_MAX_DETECTIONS);
  const bool free_now = j < n && d.owner[b0 + j] == MPE_RIG_PEEL_FREE && d.find[(size_t)i * d.n_bodies + round] != 0;
  const unsigned long long mask = __ballot(free_now);
  if (free_now) {
    const size_t at = (size_t)d.r_begin[list] + rig_peel_position(mask, j);
    d.r_xy[2 * at] = d.det_xy[2 * (size_t)(b0 + j)];
    d.r_xy[2 * at + 1] = d.det_xy[2 * (size_t)(b0 + j) + 1];
    d.map[at] = j;
  }
}

}  // namespace

hipError_t launch_k_rig_peel(const RigPeelDev& d, int round, int n_mk_prev, hipStream_t s) {
  if (d.n_problems <= 0) return hipSuccess;
  const int n_lists = d.n_problems * d.n_cam;
  const dim3 lists((unsigned)n_lists), lanes(MPE_RIG_PEEL_LANES);
  hipLaunchKernelGGL(k_rig_peel_count, lists, lanes, 0, s, d, round, n_mk_prev);
  if (round < d.n_bodies) {
    hipLaunchKernelGGL(k_rig_peel_scan, dim3(1), dim3(MPE_RIG_PEEL_SCAN_LANES), 0, s, d.counts, n_lists, d.r_begin);
    hipLaunchKernelGGL(k_rig_peel_scatter, lists, lanes, 0, s, d, round);
  }
  return hipGetLastError();
}

}  // namespace mpe
