// mpe_body_ba_plan.h — host side of mpe_body_calibrate that needs no device (plain C++, shared by mpe_body.cpp and the
// CPU tier, tests/host/body_ba_host.cpp): which rows take part (body_ba_plan) and what goes back to the caller.  The
// iteration itself is mpe_rig_ba_plan.h's (rig_ba_iterate, rig_ba_chunks) over the steps of mpe_body_ba.h.
//
// The rules, a fixed point that starts with every marker free and repeats until nothing changes:
//   * a view is USED when its rows on free markers number >= 4 and name >= 3 distinct free markers;
//   * a marker is FREE when it has >= 2 rows in used views.
// A marker that is not free is HELD: its position stays, its rows are dropped.  (Both sets only shrink, so the loop ends;
// with fewer than 3 free markers no view is used and then no marker is free.)
// Marker state: 1 calibrated, 2 held.  Scale: held when asked for, or (auto) when no used view has used rows of two
// cameras.
// Needs include/mpe.h in front (mpe_body_calibration_report).
#pragma once
#include "mpe_rig_ba_plan.h"

struct BodyBaPlan {
  int n_markers = 0, n_free = 0, views_used = 0, rows_used = 0, two_cameras = 0;
  int marker_state[16] = {}, marker_rows[16] = {}, marker_free[16] = {}, free_marker[16] = {};
  std::vector<int> used;          // per caller's view: 1 used
  std::vector<int> view_of;       // per used view: the caller's index
  std::vector<int> view_begin;    // per used view (+ 1): its rows in the compacted arrays
  std::vector<unsigned> view_mask;
  std::vector<long long> view_cum;  // doubles of the records in front of used view f (+ 1)
  std::vector<int> row_cam, row_free;
  std::vector<double> row_uv;
};

inline void body_ba_plan(int n_markers, const int* view_begin, const int* row_camera, const int* row_marker,
                         const double* row_uv, int n_views, int head_doubles, int slot_doubles, BodyBaPlan& P) {
  P = BodyBaPlan();
  P.n_markers = n_markers;
  P.used.assign((size_t)n_views, 0);
  unsigned free_set = n_markers >= 32 ? ~0u : ((1u << n_markers) - 1u);
  for (;;) {
    int rows_of[16] = {};
    for (int f = 0; f < n_views; ++f) {
      int n = 0;
      unsigned seen = 0;
      for (int j = view_begin[f]; j < view_begin[f + 1]; ++j)
        if ((free_set >> row_marker[j]) & 1u) ++n, seen |= 1u << row_marker[j];
      P.used[(size_t)f] = (n >= 4 && __builtin_popcount(seen) >= 3) ? 1 : 0;
      if (P.used[(size_t)f])
        for (int j = view_begin[f]; j < view_begin[f + 1]; ++j)
          if ((free_set >> row_marker[j]) & 1u) ++rows_of[row_marker[j]];
    }
    unsigned next = 0;
    for (int m = 0; m < n_markers; ++m)
      if (((free_set >> m) & 1u) && rows_of[m] >= 2) next |= 1u << m;
    const bool same = next == free_set;
    free_set = next;
    if (same) {
      for (int m = 0; m < n_markers; ++m) P.marker_rows[m] = ((free_set >> m) & 1u) ? rows_of[m] : 0;
      break;
    }
  }
  for (int m = 0; m < n_markers; ++m) {
    const bool is_free = (free_set >> m) & 1u;
    P.marker_state[m] = is_free ? 1 : 2;
    P.marker_free[m] = -1;
    if (is_free) {
      P.free_marker[P.n_free] = m;
      P.marker_free[m] = P.n_free++;
    }
  }
  P.view_begin.push_back(0);
  P.view_cum.push_back(0);
  for (int f = 0; f < n_views; ++f) {
    if (!P.used[(size_t)f]) continue;
    P.view_of.push_back(f);
    unsigned mask = 0, cams = 0;
    for (int j = view_begin[f]; j < view_begin[f + 1]; ++j) {
      const int fi = P.marker_free[row_marker[j]];
      if (fi < 0) continue;
      P.row_cam.push_back(row_camera[j]);
      P.row_free.push_back(fi);
      P.row_uv.insert(P.row_uv.end(), row_uv + 2 * (size_t)j, row_uv + 2 * (size_t)j + 2);
      mask |= 1u << fi;
      cams |= 1u << row_camera[j];
    }
    if (cams & (cams - 1u)) P.two_cameras = 1;
    P.view_mask.push_back(mask);
    P.view_begin.push_back((int)P.row_cam.size());
    P.view_cum.push_back(P.view_cum.back() + head_doubles + (long long)slot_doubles * __builtin_popcount(mask));
  }
  P.views_used = (int)P.view_of.size();
  P.rows_used = (int)P.row_cam.size();
}

// option scale (-1 auto, 0 free, 1 held) -> whether the seventh constraint is there
inline int body_ba_scale_held(const BodyBaPlan& P, int scale) { return scale < 0 ? (P.two_cameras ? 0 : 1) : (scale ? 1 : 0); }

// What a call hands back before anything is calibrated: the report's counts and states, every marker and view pose as
// given, a zero covariance.  (What stays when the call returns 0.)
inline void body_ba_give_back(const BodyBaPlan& P, int scale_held, const double* markers_xyz, int n_views,
                              const double* T_view_init, double* markers_out, double* T_view_out, double* cov_out,
                              int* view_used, mpe_body_calibration_report* report) {
  std::memset(report, 0, sizeof(*report));
  report->status = MPE_FRAME_NO_POSE;
  report->views_used = P.views_used;
  report->rows_used = P.rows_used;
  report->markers_free = P.n_free;
  report->scale_held = scale_held;
  for (int m = 0; m < P.n_markers; ++m) {
    report->marker_state[m] = P.marker_state[m];
    report->marker_rows[m] = P.marker_rows[m];
  }
  std::memcpy(markers_out, markers_xyz, (size_t)P.n_markers * 3 * sizeof(double));
  if (view_used)
    for (int f = 0; f < n_views; ++f) view_used[f] = P.used[(size_t)f];
  if (T_view_out && n_views > 0) std::memcpy(T_view_out, T_view_init, (size_t)n_views * 16 * sizeof(double));
  if (cov_out) std::memset(cov_out, 0, (size_t)P.n_markers * 9 * sizeof(double));
}

// The result of the iteration into the caller's arrays: markers_back (n_markers x 3, as the steps left them), T_back
// (views_used x 16), cov_back (n_free x 9).  Anything non-finite: 0, and what body_ba_give_back wrote stays.
inline int body_ba_hand_out(const BodyBaPlan& P, const RigBaOutcome& o, const double* markers_back, const double* T_back,
                            const double* cov_back, double* markers_out, double* T_view_out, double* cov_out,
                            mpe_body_calibration_report* report) {
  const int nv = P.views_used, nf = P.n_free;
  report->iterations = o.iterations;
  report->last_step = o.last_step;
  const double n_res = 2.0 * (double)P.rows_used;
  report->rms_before = std::sqrt(o.sse_before / n_res);
  report->rms_after = std::sqrt(o.sse_after / n_res);
  bool finite = std::isfinite(o.sse_before) && std::isfinite(o.sse_after) && std::isfinite(o.last_step);
  for (int i = 0; i < 3 * P.n_markers && finite; ++i) finite = std::isfinite(markers_back[i]);
  for (size_t i = 0; i < (size_t)nv * 16 && finite; ++i) finite = std::isfinite(T_back[i]);
  for (size_t i = 0; i < (size_t)nf * 9 && finite; ++i) finite = std::isfinite(cov_back[i]);
  if (!finite) return 0;
  for (int i = 0; i < nf; ++i) {
    const int m = P.free_marker[i];
    std::memcpy(markers_out + 3 * (size_t)m, markers_back + 3 * (size_t)m, 3 * sizeof(double));
    if (cov_out) std::memcpy(cov_out + 9 * (size_t)m, cov_back + 9 * (size_t)i, 9 * sizeof(double));
  }
  if (T_view_out)
    for (int v = 0; v < nv; ++v)
      std::memcpy(T_view_out + 16 * (size_t)P.view_of[(size_t)v], T_back + 16 * (size_t)v, 12 * sizeof(double));
  report->status = MPE_FRAME_POSE;
  return 1;
}
