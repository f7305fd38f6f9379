// mpe_rig_peel.h — the logic of k_rig_peel_count / k_rig_peel_scatter (mpe_rig_peel.hip): the step BETWEEN the rounds of
// mpe_rig_init_bodies_batch.  Round b finds body b in the detections no earlier body has claimed; the peel step folds the
// finished round's claims into the owner bytes, translates that round's answer from the indices of its compacted lists to
// the caller's, and compacts what is still free for the next round.  Plain C++ in a header of its own (as
// mpe_wide_peel.h is) so that the CPU tier compiles it for the host (tests/host/rig_peel_host.cpp).
//
// A camera's list holds at most MPE_MAX_DETECTIONS = 64 points — the wave width on gfx950 —, so one wave takes one
// (problem, camera) list and lane j owns detection j.  Everything here is what ONE lane does, or what one lane does for
// the whole record; the 64-bit mask of free lanes comes from __ballot on the device and from a loop on the host.
//
//   owner byte   MPE_RIG_PEEL_FREE (-1), MPE_RIG_PEEL_TAKEN (-2: claimed at entry), else the body that claimed the point
//   map          compacted index of a round -> index within the caller's list of that camera
#pragma once
#include <stdint.h>

#include "../../include/mpe.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MPE_PEEL_HD __host__ __device__ inline
#else
#define MPE_PEEL_HD inline
#endif

#define MPE_RIG_PEEL_FREE (-1)
#define MPE_RIG_PEEL_TAKEN (-2)
#define MPE_RIG_PEEL_NOT_ASKED 7  // mpe_rig_init_info.reason of a body the caller did not ask for

namespace mpe {

// Lane j's owner byte behind a finished round of body `body`: the round's match words of this camera (n_mk of them,
// 1-based within the round's compacted list, 0 none) name the detections the body claims, when the round has a pose.
// map: the round's index map of this list.
MPE_PEEL_HD int8_t rig_peel_fold(int8_t owner, int j, bool pose, const uint32_t* match, int n_mk, const int* map, int body) {
  if (!pose) return owner;
  for (int m = 0; m < n_mk; ++m) {
    const uint32_t w = match[m];
    if (w != 0 && map[w - 1] == j) owner = (int8_t)body;
  }
  return owner;
}

// the order-preserving position of free lane j among the free lanes of its list
MPE_PEEL_HD int rig_peel_position(uint64_t free_mask, int j) {
  const uint64_t below = free_mask & (((uint64_t)1 << j) - 1);  // (j <= 63)
  int n = 0;
  for (uint64_t v = below; v != 0; v &= v - 1) ++n;
  return n;
}
MPE_PEEL_HD int rig_peel_count(uint64_t free_mask) {
  int n = 0;
  for (uint64_t v = free_mask; v != 0; v &= v - 1) ++n;
  return n;
}

// a match word of a round -> the same word within the caller's list (both 1-based, 0 none)
MPE_PEEL_HD uint32_t rig_peel_word(uint32_t w, const int* map) { return w != 0 ? (uint32_t)map[w - 1] + 1u : 0u; }

// The finished round's info record for the caller: the winner's detection triple names the caller's list.  map_cam: the
// round's index map of the list of camera info.camera (unused without a winner).
MPE_PEEL_HD void rig_peel_info(const mpe_rig_init_info& in, const int* map_cam, mpe_rig_init_info* out) {
  *out = in;
  if (in.camera < 0) return;
  for (int k = 0; k < 3; ++k)
    if (in.detection[k] >= 0) out->detection[k] = map_cam[in.detection[k]];
}

// what a body that was not asked for gets: no pose, T = I, cov = 0, a zeroed info record with reason 7
MPE_PEEL_HD void rig_peel_not_asked(mpe_result* res, mpe_rig_init_info* info) {
  unsigned char* r = reinterpret_cast<unsigned char*>(res);
  for (size_t k = 0; k < sizeof(mpe_result); ++k) r[k] = 0;
  unsigned char* p = reinterpret_cast<unsigned char*>(info);
  for (size_t k = 0; k < sizeof(mpe_rig_init_info); ++k) p[k] = 0;
  for (int k = 0; k < 16; k += 5) res->T[k] = 1.0;
  res->status = MPE_FRAME_NO_POSE;
  info->reason = MPE_RIG_PEEL_NOT_ASKED;
}

}  // namespace mpe
