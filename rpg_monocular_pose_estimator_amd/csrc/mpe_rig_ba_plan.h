// mpe_rig_ba_plan.h — host side of mpe_rig_calibrate that needs no device (plain C++, shared by mpe_rig.cpp and the CPU
// tier, tests/host/rig_ba_host.cpp): which rows take part (rig_ba_plan), and the iteration itself as a sequence of the
// steps of mpe_rig_ba.h (rig_ba_iterate) over a back end that runs a step — launches on the GPU, loops over blocks on
// the host.
//
// The rules, in one pass:
//   * a view is a CANDIDATE when it has at least 3 rows and rows of at least 2 distinct cameras;
//   * cameras are linked by candidate views (an edge when a view holds rows of both); a camera outside the reference
//     camera's connected component — a camera without rows among them — is HELD: its extrinsic stays, its rows are dropped;
//   * a view is USED when it is a candidate whose cameras are in the reference camera's component (the cameras of a
//     candidate view are all in one component, so a view of held cameras holds nothing else).
// Camera state: 0 the reference camera, 1 calibrated, 2 held.
// Needs include/mpe.h in front (mpe_rig_camera, mpe_rig_calibration_report).
#pragma once
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

struct RigBaPlan {
  int n_cam = 0, n_free = 0, views_used = 0, rows_used = 0;
  int cam_state[16] = {}, cam_rows[16] = {}, cam_free[16] = {};
  std::vector<int> used;          // per caller's view: 1 used
  std::vector<int> view_of;       // per used view: the caller's index
  std::vector<int> view_begin;    // per used view (+ 1): its rows in the compacted arrays
  std::vector<unsigned> view_mask;
  std::vector<long long> view_cum;  // doubles of the records in front of used view f (+ 1)
  std::vector<int> row_cam;
  std::vector<double> row_xyz, row_uv;
};

inline void rig_ba_plan(int n_cam, int ref, const int* view_begin, const int* row_camera, const double* row_xyz,
                        const double* row_uv, int n_views, int head_doubles, int slot_doubles, RigBaPlan& P) {
  P = RigBaPlan();
  P.n_cam = n_cam;
  P.used.assign((size_t)n_views, 0);
  int parent[16];
  for (int c = 0; c < 16; ++c) parent[c] = c;
  auto find = [&](int c) {
    while (parent[c] != c) c = parent[c] = parent[parent[c]];
    return c;
  };
  std::vector<unsigned> cams_of((size_t)n_views, 0u);
  for (int f = 0; f < n_views; ++f) {
    unsigned m = 0;
    for (int j = view_begin[f]; j < view_begin[f + 1]; ++j) m |= 1u << row_camera[j];
    const bool candidate = view_begin[f + 1] - view_begin[f] >= 3 && (m & (m - 1u)) != 0;
    cams_of[(size_t)f] = candidate ? m : 0u;
    if (!candidate) continue;
    int first = -1;
    for (int c = 0; c < n_cam; ++c)
      if ((m >> c) & 1u) {
        if (first < 0) first = c;
        else parent[find(c)] = find(first);
      }
  }
  unsigned seen = 0;  // cameras with a row in a candidate view
  for (int f = 0; f < n_views; ++f) seen |= cams_of[(size_t)f];
  const int root = find(ref);
  for (int c = 0; c < n_cam; ++c) {
    const bool linked = ((seen >> c) & 1u) && ((seen >> ref) & 1u) && find(c) == root;
    P.cam_state[c] = c == ref ? 0 : (linked ? 1 : 2);
    P.cam_free[c] = -1;
    if (P.cam_state[c] == 1) P.cam_free[c] = P.n_free++;
  }
  P.view_begin.push_back(0);
  P.view_cum.push_back(0);
  for (int f = 0; f < n_views; ++f) {
    const unsigned m = cams_of[(size_t)f];
    if (!m || !((seen >> ref) & 1u)) continue;
    int any = -1;
    for (int c = 0; c < n_cam && any < 0; ++c)
      if ((m >> c) & 1u) any = c;
    if (find(any) != root) continue;
    P.used[(size_t)f] = 1;
    P.view_of.push_back(f);
    unsigned mask = 0;
    for (int j = view_begin[f]; j < view_begin[f + 1]; ++j) {
      const int c = row_camera[j];
      P.row_cam.push_back(c);
      P.row_xyz.insert(P.row_xyz.end(), row_xyz + 3 * (size_t)j, row_xyz + 3 * (size_t)j + 3);
      P.row_uv.insert(P.row_uv.end(), row_uv + 2 * (size_t)j, row_uv + 2 * (size_t)j + 2);
      ++P.cam_rows[c];
      if (P.cam_free[c] >= 0) mask |= 1u << P.cam_free[c];
    }
    P.view_mask.push_back(mask);
    P.view_begin.push_back((int)P.row_cam.size());
    P.view_cum.push_back(P.view_cum.back() + head_doubles + (long long)slot_doubles * __builtin_popcount(mask));
  }
  P.views_used = (int)P.view_of.size();
  P.rows_used = (int)P.row_cam.size();
}

// the used views cut into chunks whose records hold at most cap_doubles (a view alone may pass it): [first, first + count)
template <class Plan>  // (RigBaPlan, or mpe_body_ba_plan.h's)
inline std::vector<std::pair<int, int>> rig_ba_chunks(const Plan& P, long long cap_doubles) {
  std::vector<std::pair<int, int>> out;
  int first = 0;
  for (int f = 0; f < P.views_used; ++f) {
    if (f > first && P.view_cum[(size_t)f + 1] - P.view_cum[(size_t)first] > cap_doubles) {
      out.push_back({first, f - first});
      first = f;
    }
  }
  if (P.views_used > first) out.push_back({first, P.views_used - first});
  return out;
}

struct RigBaOutcome {
  int iterations = 0;
  double sse_before = 0, sse_after = 0, last_step = 0;
};

// Gauss-Newton over the steps of a back end B:
//   B.linearise(first, count), B.reduce(first, count, restart), B.solve(), B.update(first, count),
//   B.finish(apply, out2) -> 0 or an error code (out2 = [largest |step|, sum of squared residuals]), B.covariance().
// With one chunk the records of the linearisation are still there for the update; with several every chunk is linearised
// a second time (the same values: nothing it reads has changed) in front of its update.  Stop: the largest |step| <=
// tolerance (a NaN step stops too), or max_iterations.  The residuals are evaluated once more at the final values.
template <class Backend>
int rig_ba_iterate(Backend& B, const std::vector<std::pair<int, int>>& chunks, int max_iterations, double tolerance,
                   RigBaOutcome& o) {
  int rc = 0;
  double out2[2] = {0, 0};
  for (int it = 0; it < max_iterations; ++it) {
    for (size_t c = 0; c < chunks.size(); ++c) {
      if ((rc = B.linearise(chunks[c].first, chunks[c].second))) return rc;
      if ((rc = B.reduce(chunks[c].first, chunks[c].second, c == 0))) return rc;
    }
    if ((rc = B.solve())) return rc;
    for (size_t c = 0; c < chunks.size(); ++c) {
      if (chunks.size() > 1 && (rc = B.linearise(chunks[c].first, chunks[c].second))) return rc;
      if ((rc = B.update(chunks[c].first, chunks[c].second))) return rc;
    }
    if ((rc = B.finish(1, out2))) return rc;
    if (it == 0) o.sse_before = out2[1];
    o.iterations = it + 1;
    o.last_step = out2[0];
    if (!(out2[0] > tolerance)) break;
  }
  if ((rc = B.covariance())) return rc;
  for (size_t c = 0; c < chunks.size(); ++c)
    if ((rc = B.linearise(chunks[c].first, chunks[c].second))) return rc;
  if ((rc = B.finish(0, out2))) return rc;
  o.sse_after = out2[1];
  return 0;
}

// What a call hands back before anything is calibrated: the report's counts and states, every extrinsic and view pose as
// given, a zero covariance.  (What stays when the call returns 0.)
inline void rig_ba_give_back(const RigBaPlan& P, const mpe_rig_camera* cameras, int n_views, const double* T_view_init,
                             double* T_cam_rig_out, double* T_view_out, double* cov_out, int* view_used,
                             mpe_rig_calibration_report* report) {
  std::memset(report, 0, sizeof(*report));
  report->status = MPE_FRAME_NO_POSE;
  report->views_used = P.views_used;
  report->rows_used = P.rows_used;
  for (int c = 0; c < P.n_cam; ++c) {
    report->camera_state[c] = P.cam_state[c];
    report->camera_rows[c] = P.cam_rows[c];
    std::memcpy(T_cam_rig_out + 16 * (size_t)c, cameras[c].T_cam_rig, 16 * sizeof(double));
  }
  if (view_used)
    for (int f = 0; f < n_views; ++f) view_used[f] = P.used[(size_t)f];
  if (T_view_out && n_views > 0) std::memcpy(T_view_out, T_view_init, (size_t)n_views * 16 * sizeof(double));
  if (cov_out) std::memset(cov_out, 0, (size_t)P.n_cam * 36 * sizeof(double));
}

// The result of the iteration into the caller's arrays: cam_back (n_cam, the extrinsics as the steps left them), T_back
// (views_used x 16), cov_back (n_free x 36).  Anything non-finite: 0, and what rig_ba_give_back wrote stays.
inline int rig_ba_hand_out(const RigBaPlan& P, const RigBaOutcome& o, const mpe_rig_camera* cam_back, const double* T_back,
                           const double* cov_back, double* T_cam_rig_out, double* T_view_out, double* cov_out,
                           mpe_rig_calibration_report* report) {
  const int nv = P.views_used, nf = P.n_free;
  report->iterations = o.iterations;
  report->last_step = o.last_step;
  const double n_res = 2.0 * (double)P.rows_used;
  report->rms_before = std::sqrt(o.sse_before / n_res);
  report->rms_after = std::sqrt(o.sse_after / n_res);
  bool finite = std::isfinite(o.sse_before) && std::isfinite(o.sse_after) && std::isfinite(o.last_step);
  for (int c = 0; c < P.n_cam && finite; ++c)
    for (int i = 0; i < 12; ++i) finite = finite && std::isfinite(cam_back[c].T_cam_rig[i]);
  for (size_t i = 0; i < (size_t)nv * 16 && finite; ++i) finite = std::isfinite(T_back[i]);
  for (size_t i = 0; i < (size_t)nf * 36 && finite; ++i) finite = std::isfinite(cov_back[i]);
  if (!finite) return 0;
  for (int c = 0; c < P.n_cam; ++c) {
    if (P.cam_state[c] != 1) continue;
    std::memcpy(T_cam_rig_out + 16 * (size_t)c, cam_back[c].T_cam_rig, 12 * sizeof(double));
    if (cov_out) std::memcpy(cov_out + 36 * (size_t)c, cov_back + 36 * (size_t)P.cam_free[c], 36 * sizeof(double));
  }
  if (T_view_out)
    for (int v = 0; v < nv; ++v)
      std::memcpy(T_view_out + 16 * (size_t)P.view_of[(size_t)v], T_back + 16 * (size_t)v, 12 * sizeof(double));
  report->status = MPE_FRAME_POSE;
  return 1;
}
