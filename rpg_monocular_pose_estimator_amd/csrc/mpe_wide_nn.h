// mpe_wide_nn.h — the logic of k_nn_wide (mpe_k3.hip): findCorrespondences (pose_estimator.cpp:372-392, 862-906) over a
// detection set of up to MPE_WIDE_DETECTIONS points, with exactly the arithmetic of the narrow tracked path (k3a_body):
// du = pu - x_j, dv = pv - y_j, d2 = du*du + dv*dv without contraction, strict `<` over ascending j (the lowest index
// among equal minima wins, a NaN d2 never wins), bj = 0 when nothing won, the row kept iff sqrt(best) <= nn_tol, rows in
// ascending marker order.  Plain C++ in a header of its own (as mpe_wide_peel.h is) so that the CPU tier compiles it for
// the host (tests/host/wide_nn_host.cpp) and runs it under AddressSanitizer against the plain double loop.
//
// The parallel form is one wave per item: lane l holds detections l, l + 64, l + 128, l + 192 in registers and reduces
// them in ascending j (wide_nn_lane), then the wave reduces the pairs (d2, index) with wide_nn_better — smaller d2 wins,
// equal d2 goes to the smaller index, NaN (carried as "nothing won": index 0) loses.  That order is total on the pairs
// that can occur (every index > 0 is held by exactly one lane), so any reduction tree gives the sequential loop's answer.
//
// Detection indices reach 256 in 1-based form: everything here holds them in `unsigned`, never in a byte.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/mpe.h"
#include "mpe_wide_peel.h"  // (MPE_WIDE_HD, wide_compact_rows)

namespace mpe {

#define MPE_WIDE_NN_PER_LANE (MPE_WIDE_DETECTIONS / 64)

// The best of one lane's detections for the predicted pixel (pu, pv): lx / ly hold detections lane, lane + 64, ... (entry
// k valid iff lane + 64 k < n_d).  best = +inf and bj = 0 when nothing won.
MPE_WIDE_HD void wide_nn_lane(const double* lx, const double* ly, int lane, int n_d, double pu, double pv, double& best,
                              unsigned& bj) {
  best = (double)INFINITY;
  bj = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < MPE_WIDE_NN_PER_LANE; ++k) {
    const int j = lane + 64 * k;
    if (j >= n_d) continue;
    const double du = pu - lx[k], dv = pv - ly[k];
    const double d2 = du * du + dv * dv;
    if (d2 < best) {
      best = d2;
      bj = (unsigned)j + 1u;
    }
  }
}

// does the pair (d2b, jb) beat (d2a, ja)?  Index 0 = nothing won (its d2 is +inf): it never beats, and anything that won
// beats it — a detection AT distance +inf does not exist, since `d2 < inf` had to hold for it to win.
MPE_WIDE_HD bool wide_nn_better(double d2b, unsigned jb, double d2a, unsigned ja) {
  if (jb == 0u) return false;
  if (ja == 0u) return true;
  return d2b < d2a || (d2b == d2a && jb < ja);
}

// the row test of findCorrespondences (sqrt(+inf) <= tol is false for every finite tol, NaN tol keeps nothing).  A
// marker for which nothing won names no detection: with an infinite tolerance it still makes no row here (the
// compaction below indexes the record through every row).
MPE_WIDE_HD bool wide_nn_keep(double best, unsigned bj, double nn_tol) { return bj != 0u && sqrt(best) <= nn_tol; }

// The sequential form, over a record's interleaved coordinates: rows (marker, detection), 1-based, to cm / cd (n_markers
// entries each at most); returns their number.
MPE_WIDE_HD int wide_nn_rows(const double* pred_px, int n_markers, const double* det_xy, int n_d, double nn_tol,
                             unsigned* cm, unsigned* cd) {
  int n_c = 0;
  for (int i = 0; i < n_markers; ++i) {
    double best = (double)INFINITY;
    unsigned bj = 0u;
    const double pu = pred_px[2 * i], pv = pred_px[2 * i + 1];
    for (int j = 0; j < n_d; ++j) {
      const double du = pu - det_xy[2 * j], dv = pv - det_xy[2 * j + 1];
      const double d2 = du * du + dv * dv;
      if (d2 < best) {
        best = d2;
        bj = (unsigned)j + 1u;
      }
    }
    if (wide_nn_keep(best, bj, nn_tol)) {
      cm[n_c] = (unsigned)i + 1u;
      cd[n_c] = bj;
      ++n_c;
    }
  }
  return n_c;
}

// The hand-over to the validate / refine kernels, as k3_peel_wide makes it: the detections the n_c rows name compacted
// into an ordinary record (one slot for a detection named by two markers, padded to four slots with copies of the first:
// k3a_body asks for 4 before it parses given rows, and nothing reads a detection no row names), the rows re-indexed into
// it (corr_compact: 2 * MPE_MAX_MARKERS words, 0-terminated), the wide index (1-based) of every slot (slot_wide:
// MPE_MAX_MARKERS words).  n_c == 0: the empty record and no rows — the tail reports status 1.  `status` is the wide
// record's.
MPE_WIDE_HD void wide_hand_over(const mpe_detections_wide* d, const unsigned* cm, const unsigned* cd, int n_c,
                                mpe_detections* o, uint32_t* corr_compact, uint32_t* slot_wide) {
  unsigned sw[MPE_MAX_MARKERS], cs[MPE_MAX_MARKERS];
  const int n_s = wide_compact_rows(cd, n_c, sw, cs);
  const int n_o = n_s == 0 ? 0 : (n_s < 4 ? 4 : n_s);
  o->n = n_o;
  o->status = d->status;
  for (int k = 0; k < n_o; ++k) {
    const int w = (int)sw[k < n_s ? k : 0] - 1;
    o->undist_xy[2 * k] = d->undist_xy[2 * w];
    o->undist_xy[2 * k + 1] = d->undist_xy[2 * w + 1];
    o->dist_xy[2 * k] = d->dist_xy[2 * w];
    o->dist_xy[2 * k + 1] = d->dist_xy[2 * w + 1];
  }
  for (int i = 0; i < MPE_MAX_MARKERS; ++i) {
    corr_compact[2 * i] = i < n_c ? cm[i] : 0u;
    corr_compact[2 * i + 1] = i < n_c ? cs[i] : 0u;
    slot_wide[i] = sw[i];
  }
}

}  // namespace mpe
