// mpe_wide_peel.h — the logic of k3_peel_wide (mpe_k3.hip): correspondencesFromHistogram (pose_estimator.cpp:344-370) over
// the vote histogram of a detection set of up to MPE_WIDE_DETECTIONS points, and the compaction of the detections its
// rows name into an ordinary mpe_detections record for the validate / refine kernels.  Plain C++ in a header of its own
// (as mpe_gather.h and mpe_brute_blocks.h are) so that the CPU tier compiles it for the host
// (tests/host/wide_peel_host.cpp) and runs it under AddressSanitizer against the oracle.
//
// Detection indices reach 256 in 1-based form: everything here holds them in `unsigned`, never in a byte.
#pragma once
#include <stdint.h>

#include "../../include/mpe.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MPE_WIDE_HD __host__ __device__ inline
#else
#define MPE_WIDE_HD inline
#endif

namespace mpe {

// Column c of a histogram of n_det rows of MPE_MAX_MARKERS words: its maximum and the first row that reaches it (an
// all-zero column keeps row 0, as the reference's scan does when histogram_threshold is 0).
MPE_WIDE_HD void wide_column_max(const uint32_t* H, int n_det, int c, unsigned& max_out, unsigned& row_out) {
  unsigned mv = 0, mr = 0;
  for (int r = 0; r < n_det; ++r) {
    const unsigned v = H[(size_t)r * MPE_MAX_MARKERS + c];
    if (v > mv) {
      mv = v;
      mr = (unsigned)r;
    }
  }
  max_out = mv;
  row_out = mr;
}

// initialise()'s all-zero test (pose_estimator.cpp:704) and correspondencesFromHistogram from the column maxima.  The
// reference scans the whole histogram n_markers times, column-major, for the first position of the strict maximum and
// then zeroes that COLUMN: only columns are ever removed, so a column's maximum and its first row never change, and a
// round is the first column, in ascending order, with the largest value still standing (k3a_body peels the narrow
// histogram the same way).  A removed column stands at 0 with row 0.  Rows (marker, detection), 1-based, go to cm / cd
// (n_markers entries each at most); returns their number.  One detection may be named by several markers.
MPE_WIDE_HD int wide_peel_rows(const unsigned* colmax, const unsigned* colrow, int n_markers, unsigned hist_thr,
                               unsigned* cm, unsigned* cd) {
  bool any = false;
  for (int c = 0; c < n_markers; ++c) any |= (colmax[c] != 0);
  if (!any) return 0;
  unsigned removed = 0;  // zeroed columns (n_markers <= MPE_MAX_MARKERS = 16)
  int n_c = 0;
  for (int j = 0; j < n_markers; ++j) {
    unsigned mv = 0, ri = 0;
    int ci = 0;
    bool first = true;
    for (int c = 0; c < n_markers; ++c) {
      const bool gone = (removed >> c) & 1u;
      const unsigned v = gone ? 0u : colmax[c];
      if (first || v > mv) {
        mv = v;
        ri = gone ? 0u : colrow[c];
        ci = c;
        first = false;
      }
    }
    if (mv < hist_thr) break;
    cm[n_c] = (unsigned)ci + 1u;
    cd[n_c] = ri + 1u;
    ++n_c;
    removed |= 1u << ci;
  }
  return n_c;
}

// The detections the n_c rows name, compacted: distinct detections get distinct slots in ascending wide index, a
// detection named twice shares one slot.  slot_wide[s] = wide index (1-based) of slot s (MPE_MAX_MARKERS entries, 0
// beyond the slots), cslot[i] = slot (1-based) of row i's detection.  Returns the number of slots (<= n_c).
MPE_WIDE_HD int wide_compact_rows(const unsigned* cd, int n_c, unsigned* slot_wide, unsigned* cslot) {
  int n_s = 0;
  for (int i = 0; i < n_c; ++i) {  // insertion into the sorted list of distinct indices (n_c <= 16)
    const unsigned d = cd[i];
    int k = 0;
    while (k < n_s && slot_wide[k] < d) ++k;
    if (k < n_s && slot_wide[k] == d) continue;
    for (int m = n_s; m > k; --m) slot_wide[m] = slot_wide[m - 1];
    slot_wide[k] = d;
    ++n_s;
  }
  for (int k = n_s; k < MPE_MAX_MARKERS; ++k) slot_wide[k] = 0;
  for (int i = 0; i < n_c; ++i) {
    int k = 0;
    while (slot_wide[k] != cd[i]) ++k;  // (present by construction)
    cslot[i] = (unsigned)k + 1u;
  }
  return n_s;
}

}  // namespace mpe
