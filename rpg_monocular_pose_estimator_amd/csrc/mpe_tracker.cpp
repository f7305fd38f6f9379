// mpe_tracker.cpp — the stateful PoseEstimator state machine (tracking path) on top of the HIP
// stages.  Host side only: a few 4x4 / 6-vector operations per frame; all image and pose compute
// runs in the kernels.  One state machine (BatchCtx) serves one stream and
// N streams in lock step alike: its device steps are the lock-step submissions
// (submit_tracked, mpe_host.h / mpe_track_step_batch_collect: detection in the ROI with correspondences,
// validation and refinement) and mpe_solve_bruteforce_batch (re-initialisation); with
// mpe_tracker_set_wide_frames, frames of 65 .. MPE_WIDE_DETECTIONS detections repeat those two steps
// through mpe_track_step_batch_wide and mpe_solve_bruteforce_batch_wide.
//
// Reference: PoseEstimator::estimateBodyPose (pose_estimator.cpp:62-147), predictPose (:232-244),
// predictMarkerPositionsInImage (:270-276), findCorrespondences (:372-392), updatePose /
// optimiseAndUpdatePose / predictWithROI / findCorrespondencesAndPredictPose (:794-848),
// logarithmMap / exponentialMap (:962-1064), LEDDetector::determineROI / distortPoints
// (led_detector.cpp:114-224).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "mpe_host.h"   // (SlotPixels, submit_tracked, set_error)
#include "mpe_pixel.h"  // (check_image_format, same_image_format)

namespace {

struct Mat4 {
  double a[4][4];
};

Mat4 eye4() {
  Mat4 m;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) m.a[i][j] = i == j ? 1.0 : 0.0;
  return m;
}

Mat4 matmul(const Mat4& x, const Mat4& y) {
  Mat4 r;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = 0;
      for (int k = 0; k < 4; ++k) s += x.a[i][k] * y.a[k][j];
      r.a[i][j] = s;
    }
  return r;
}

// general inverse (Gauss-Jordan, partial pivoting) — Eigen's Matrix4d::inverse() in the reference
Mat4 inverse(const Mat4& m) {
  double w[4][8];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      w[i][j] = m.a[i][j];
      w[i][4 + j] = i == j ? 1.0 : 0.0;
    }
  for (int c = 0; c < 4; ++c) {
    int piv = c;
    for (int r = c + 1; r < 4; ++r)
      if (std::fabs(w[r][c]) > std::fabs(w[piv][c])) piv = r;
    if (piv != c)
      for (int j = 0; j < 8; ++j) std::swap(w[c][j], w[piv][j]);
    const double d = w[c][c];
    for (int j = 0; j < 8; ++j) w[c][j] /= d;
    for (int r = 0; r < 4; ++r) {
      if (r == c) continue;
      const double f = w[r][c];
      for (int j = 0; j < 8; ++j) w[r][j] -= f * w[c][j];
    }
  }
  Mat4 out;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) out.a[i][j] = w[i][4 + j];
  return out;
}

// pose_estimator.cpp:962-994
Mat4 exp_se3(const double tw[6]) {
  const double wx = tw[3], wy = tw[4], wz = tw[5];
  const double theta = std::sqrt(wx * wx + wy * wy + wz * wz), th2 = theta * theta;
  const double O[3][3] = {{0, -wz, wy}, {wz, 0, -wx}, {-wy, wx, 0}};
  double O2[3][3], R[3][3], V[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) O2[i][j] = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double I = i == j ? 1.0 : 0.0;
      if (theta == 0) {
        R[i][j] = V[i][j] = I;
      } else {
        R[i][j] = I + O[i][j] / theta * std::sin(theta) + O2[i][j] / th2 * (1 - std::cos(theta));
        V[i][j] = I + (1 - std::cos(theta)) / th2 * O[i][j] + (theta - std::sin(theta)) / (th2 * theta) * O2[i][j];
      }
    }
  Mat4 T = eye4();
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T.a[i][j] = R[i][j];
    T.a[i][3] = V[i][0] * tw[0] + V[i][1] * tw[1] + V[i][2] * tw[2];
  }
  return T;
}

// pose_estimator.cpp:996-1064
void log_se3(const Mat4& T, double xi[6]) {
  double what[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  double dev = 0, nr = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double e = T.a[i][j] - (i == j ? 1.0 : 0.0);
      dev += e * e;
      nr += T.a[i][j] * T.a[i][j];
    }
  // Eigen isApprox(Identity, 1e-10): squared distance <= prec^2 * min(squared norms)
  if (!(dev <= 1e-20 * std::min(nr, 3.0))) {
    double c = (T.a[0][0] + T.a[1][1] + T.a[2][2] - 1) / 2;
    c = c > 1 ? 1 : (c < -1 ? -1 : c);
    const double phi = std::acos(c);
    if (phi != 0)
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) what[i][j] = (T.a[i][j] - T.a[j][i]) / (2 * std::sin(phi)) * phi;
  }
  const double w[3] = {what[2][1], what[0][2], what[1][0]};
  const double wn = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double t[3] = {T.a[0][3], T.a[1][3], T.a[2][3]};
  double Ai[3][3];
  if (t[0] == 0 && t[1] == 0 && t[2] == 0) {  // isApproxToConstant(0, 1e-10) holds only for exact zeros
    std::memset(Ai, 0, sizeof(Ai));
  } else if (wn == 0 || std::sin(wn) == 0) {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) Ai[i][j] = i == j ? 1.0 : 0.0;
  } else {
    const double k = (2 * std::sin(wn) - wn * (1 + std::cos(wn))) / (2 * wn * wn * std::sin(wn));
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        const double sq = what[i][0] * what[0][j] + what[i][1] * what[1][j] + what[i][2] * what[2][j];
        Ai[i][j] = (i == j ? 1.0 : 0.0) - what[i][j] / 2 + k * sq;
      }
  }
  for (int i = 0; i < 3; ++i) {
    xi[i] = Ai[i][0] * t[0] + Ai[i][1] * t[1] + Ai[i][2] * t[2];
    xi[3 + i] = w[i];
  }
}

// predictPose, pose_estimator.cpp:232-244
Mat4 predict_pose(const Mat4& current, const Mat4& previous, double t_current, double t_previous, double t_predicted) {
  double delta[6], dh[6];
  log_se3(matmul(inverse(previous), current), delta);
  for (int i = 0; i < 6; ++i) dh[i] = delta[i] / (t_current - t_previous) * (t_predicted - t_current);
  return matmul(current, exp_se3(dh));
}

// project2d, pose_estimator.cpp:251-268: (K [I|0] * T) * point, evaluated left to right like the reference
void project_point(const double K[9], const Mat4& T, const double* m, double& u, double& v) {
  double t[3];
  for (int i = 0; i < 3; ++i) {
    double ct[4];
    for (int j = 0; j < 4; ++j) {
      double s = K[3 * i] * T.a[0][j];
      s += K[3 * i + 1] * T.a[1][j];
      s += K[3 * i + 2] * T.a[2][j];
      s += 0.0 * T.a[3][j];
      ct[j] = s;
    }
    double s = ct[0] * m[0];
    s += ct[1] * m[1];
    s += ct[2] * m[2];
    s += ct[3] * 1.0;
    t[i] = s;
  }
  u = t[0] / t[2];
  v = t[1] / t[2];
}

// findCorrespondences, pose_estimator.cpp:372-392: nearest detection of every predicted marker pixel
// (first minimum wins), kept if within the tolerance.  corr: rows (marker, detection), 1-based.
int find_correspondences(const double* pred_px, int n_markers, const double* det_xy, int n_det, double tol,
                         uint32_t* corr) {
  int nc = 0;
  for (int i = 0; i < n_markers; ++i) {
    double best = std::numeric_limits<double>::infinity();
    unsigned bj = 0;
    for (int j = 0; j < n_det; ++j) {
      const double du = pred_px[2 * i] - det_xy[2 * j], dv = pred_px[2 * i + 1] - det_xy[2 * j + 1];
      const double d2 = du * du + dv * dv;
      if (d2 < best) {
        best = d2;
        bj = (unsigned)j + 1;
      }
    }
    if (std::sqrt(best) <= tol) {
      corr[2 * nc] = (unsigned)i + 1;
      corr[2 * nc + 1] = bj;
      ++nc;
    }
  }
  return nc;
}

struct BatchCtx;
}  // namespace

struct mpe_tracker {
  mpe_handle* h = nullptr;
  mpe_params p;
  double K[9];
  std::vector<double> D;
  std::vector<double> markers;  // n x 3
  Mat4 current, previous, predicted;
  double cov[36];
  double t_current = 0, t_previous = 0, t_predicted = 0;
  unsigned it_since_initialized = 0;
  int roi[4] = {0, 0, 0, 0};
  bool pose_updated = false;
  std::vector<double> predicted_px;  // n_markers x 2
  std::vector<double> det;           // detected_led_positions of the current call
  std::vector<float> det_dist;       // distorted_detection_centers_ (always rewritten by a detection)
  std::vector<uint32_t> corr;        // rows (marker, detection)
  int n_corr = 0, gn_iterations = 0;
  bool used_bruteforce = false;
  bool wide_frames = false;  // mpe_tracker_set_wide_frames
  BatchCtx* solo = nullptr;  // mpe_tracker_estimate's lock-step group of one, kept for its buffers
  ~mpe_tracker();
};

namespace {

int n_markers(const mpe_tracker* t) { return (int)(t->markers.size() / 3); }

void project(const mpe_tracker* t, const Mat4& T, const double* m, double& u, double& v) {
  project_point(t->K, T, m, u, v);
}

// LEDDetector::distortPoints for one point, float in / float out (led_detector.cpp:181-224)
void distort_point(const double K[9], const double* D, int nD, float sx, float sy, float& ox, float& oy) {
  const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  const double k1 = nD > 0 ? D[0] : 0, k2 = nD > 1 ? D[1] : 0, p1 = nD > 2 ? D[2] : 0, p2 = nD > 3 ? D[3] : 0,
               k3 = nD > 4 ? D[4] : 0;
  const double x = ((double)sx - cx) / fx, y = ((double)sy - cy) / fy;
  const double r2 = x * x + y * y;
  double xc = x * (1. + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2);
  double yc = y * (1. + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2);
  xc = xc + (2. * p1 * x * y + p2 * (r2 + 2. * x * x));
  yc = yc + (p1 * (r2 + 2. * y * y) + 2. * p2 * x * y);
  ox = (float)(xc * fx + cx);
  oy = (float)(yc * fy + cy);
}

// LEDDetector::determineROI (led_detector.cpp:114-179)
void determine_roi_impl(const double* px, int n, int rows, int cols, int border, const double K[9], const double* D,
                        int nD, int roi[4]) {
  double x_min = std::numeric_limits<double>::infinity(), x_max = 0, y_min = x_min, y_max = 0;
  for (int i = 0; i < n; ++i) {
    const double u = px[2 * i], v = px[2 * i + 1];
    if (u < x_min) x_min = u;
    if (u > x_max) x_max = u;
    if (v < y_min) y_min = v;
    if (v > y_max) y_max = v;
  }
  float ax, ay, bx, by;
  distort_point(K, D, nD, (float)x_min, (float)y_min, ax, ay);
  distort_point(K, D, nD, (float)x_max, (float)y_max, bx, by);
  const double x0 = std::max(0.0, std::min((double)cols, (double)ax - border));
  const double x1 = std::max(0.0, std::min((double)cols, (double)bx + border));
  const double y0 = std::max(0.0, std::min((double)rows, (double)ay - border));
  const double y1 = std::max(0.0, std::min((double)rows, (double)by + border));
  if (x1 - x0 < 1 || y1 - y0 < 1) {
    roi[0] = 0;
    roi[1] = 0;
    roi[2] = cols;
    roi[3] = rows;
  } else {
    roi[0] = (int)x0;
    roi[1] = (int)y0;
    roi[2] = (int)(x1 - x0);
    roi[3] = (int)(y1 - y0);
  }
}

void determine_roi(mpe_tracker* t, int rows, int cols) {
  determine_roi_impl(t->predicted_px.data(), n_markers(t), rows, cols, (int)t->p.roi_border_thickness, t->K,
                     t->D.empty() ? nullptr : t->D.data(), (int)t->D.size(), t->roi);
}

void take_result(mpe_tracker* t, const mpe_result& r) {
  std::memcpy(t->predicted.a, r.T, sizeof(r.T));
  std::memcpy(t->cov, r.cov, sizeof(r.cov));
  t->gn_iterations = r.gn_iterations;
  // optimiseAndUpdatePose (pose_estimator.cpp:802-812) + updatePose (:794-800)
  if (t->it_since_initialized < 2) t->it_since_initialized++;
  t->previous = t->current;
  t->current = t->predicted;
  t->t_previous = t->t_current;
  t->t_current = t->t_predicted;
  t->pose_updated = true;
}

}  // namespace

extern "C" {

int mpe_determine_roi(const double* pixel_positions, int n_points, int rows, int cols, int border_size, const double K[9],
                      const double* D, int nD, int roi_xywh[4]) {
  if (!pixel_positions || n_points <= 0 || !K || !roi_xywh || rows <= 0 || cols <= 0 || nD < 0 || (nD > 0 && !D))
    return MPE_ERR_ARG;
  determine_roi_impl(pixel_positions, n_points, rows, cols, border_size, K, D, nD, roi_xywh);
  return MPE_OK;
}

int mpe_distort_points(const float* src_xy, float* dst_xy, int n, const double K[9], const double* D, int nD) {
  if (n < 0 || (n > 0 && (!src_xy || !dst_xy)) || !K || nD < 0 || (nD > 0 && !D)) return MPE_ERR_ARG;
  for (int i = 0; i < n; ++i) distort_point(K, D, nD, src_xy[2 * i], src_xy[2 * i + 1], dst_xy[2 * i], dst_xy[2 * i + 1]);
  return MPE_OK;
}

int mpe_exponential_map(const double twist[6], double T[16]) {
  if (!twist || !T) return MPE_ERR_ARG;
  const Mat4 m = exp_se3(twist);
  std::memcpy(T, m.a, sizeof(m.a));
  return MPE_OK;
}

int mpe_logarithm_map(const double T[16], double twist[6]) {
  if (!twist || !T) return MPE_ERR_ARG;
  Mat4 m;
  std::memcpy(m.a, T, sizeof(m.a));
  log_se3(m, twist);
  return MPE_OK;
}

int mpe_predict_pose(const double current_pose[16], const double previous_pose[16], double current_time,
                     double previous_time, double time_to_predict, double predicted_pose[16]) {
  if (!current_pose || !previous_pose || !predicted_pose) return MPE_ERR_ARG;
  Mat4 c, pr;
  std::memcpy(c.a, current_pose, sizeof(c.a));
  std::memcpy(pr.a, previous_pose, sizeof(pr.a));
  const Mat4 out = predict_pose(c, pr, current_time, previous_time, time_to_predict);
  std::memcpy(predicted_pose, out.a, sizeof(out.a));
  return MPE_OK;
}

int mpe_project_points(const double T[16], const double* markers_xyz, int n, const double K[9], double* px) {
  if (!T || !K || n < 0 || (n > 0 && (!markers_xyz || !px))) return MPE_ERR_ARG;
  Mat4 m;
  std::memcpy(m.a, T, sizeof(m.a));
  for (int i = 0; i < n; ++i) project_point(K, m, markers_xyz + 3 * i, px[2 * i], px[2 * i + 1]);
  return MPE_OK;
}

int mpe_find_correspondences(const double* predicted_px, int n_markers, const double* det_xy, int n_det,
                             double nearest_neighbour_pixel_tolerance, uint32_t* corr) {
  if (n_markers < 0 || n_det < 0 || (n_markers > 0 && (!predicted_px || !corr)) || (n_det > 0 && !det_xy))
    return MPE_ERR_ARG;
  return find_correspondences(predicted_px, n_markers, det_xy, n_det, nearest_neighbour_pixel_tolerance, corr);
}

int mpe_tracker_get_state(const mpe_tracker* t, mpe_tracker_state* st) {
  if (!t || !st) return MPE_ERR_ARG;
  std::memcpy(st->current_pose, t->current.a, sizeof(st->current_pose));
  std::memcpy(st->previous_pose, t->previous.a, sizeof(st->previous_pose));
  std::memcpy(st->predicted_pose, t->predicted.a, sizeof(st->predicted_pose));
  std::memcpy(st->pose_covariance, t->cov, sizeof(st->pose_covariance));
  st->current_time = t->t_current;
  st->previous_time = t->t_previous;
  st->predicted_time = t->t_predicted;
  st->it_since_initialized = t->it_since_initialized;
  for (int i = 0; i < 4; ++i) st->roi[i] = t->roi[i];
  return MPE_OK;
}

int mpe_tracker_set_state(mpe_tracker* t, const mpe_tracker_state* st) {
  if (!t || !st) return MPE_ERR_ARG;
  std::memcpy(t->current.a, st->current_pose, sizeof(st->current_pose));
  std::memcpy(t->previous.a, st->previous_pose, sizeof(st->previous_pose));
  std::memcpy(t->predicted.a, st->predicted_pose, sizeof(st->predicted_pose));
  std::memcpy(t->cov, st->pose_covariance, sizeof(st->pose_covariance));
  t->t_current = st->current_time;
  t->t_previous = st->previous_time;
  t->t_predicted = st->predicted_time;
  t->it_since_initialized = st->it_since_initialized;
  for (int i = 0; i < 4; ++i) t->roi[i] = st->roi[i];
  return MPE_OK;
}

int mpe_tracker_create(mpe_handle* h, mpe_tracker** out) {
  if (!h || !out) return MPE_ERR_ARG;
  mpe_tracker* t = new mpe_tracker();
  t->h = h;
  mpe_default_params(&t->p);
  t->p.back_projection_pixel_tolerance = 3;    // constructor defaults, pose_estimator.cpp:34-42
  t->p.nearest_neighbour_pixel_tolerance = 5;
  t->p.certainty_threshold = 0.75;
  t->p.valid_correspondence_threshold = 0.7;
  std::memset(t->K, 0, sizeof(t->K));
  t->current = t->previous = t->predicted = eye4();
  std::memset(t->cov, 0, sizeof(t->cov));
  *out = t;
  return MPE_OK;
}

void mpe_tracker_destroy(mpe_tracker* t) { delete t; }

int mpe_tracker_set_markers(mpe_tracker* t, const double* xyz, int n) {
  if (!t || (!xyz && n > 0) || n < 0 || n > MPE_MAX_MARKERS) return MPE_ERR_ARG;
  t->markers.assign(xyz, xyz + 3 * n);
  t->predicted_px.assign(2 * n, 0.0);
  t->p.histogram_threshold = 0;  // numCombinations(n,3), pose_estimator.cpp:54
  return MPE_OK;
}

int mpe_tracker_set_camera(mpe_tracker* t, const double K[9], const double* D, int nD) {
  if (!t || !K || nD < 0 || (nD > 0 && !D)) return MPE_ERR_ARG;
  std::memcpy(t->K, K, sizeof(t->K));
  if (nD > 0)
    t->D.assign(D, D + nD);
  else
    t->D.clear();
  return MPE_OK;
}

int mpe_tracker_set_params(mpe_tracker* t, const mpe_params* p) {
  if (!t || !p) return MPE_ERR_ARG;
  t->p = *p;
  return MPE_OK;
}

int mpe_tracker_set_wide_frames(mpe_tracker* t, int on) {
  if (!t) return MPE_ERR_ARG;
  t->wide_frames = on != 0;
  return MPE_OK;
}

int mpe_tracker_reset(mpe_tracker* t) {
  if (!t) return MPE_ERR_ARG;
  t->it_since_initialized = 0;
  if (t->h) (void)mpe_track_step_batch_cancel(t->h);  // (a submission abandoned by a failed batch call)
  return MPE_OK;
}

int mpe_tracker_get_correspondences(mpe_tracker* t, uint32_t* corr, int cap_rows) {  // getCorrespondences()
  if (!t || (!corr && cap_rows > 0)) return MPE_ERR_ARG;
  const int n = std::min<int>((int)t->corr.size() / 2, cap_rows);
  for (int i = 0; i < 2 * n; ++i) corr[i] = t->corr[i];
  return (int)t->corr.size() / 2;
}

int mpe_tracker_get_image_points(mpe_tracker* t, double* xy, int cap_points) {  // getImagePoints()
  if (!t || (!xy && cap_points > 0)) return MPE_ERR_ARG;
  const int n = std::min<int>((int)t->det.size() / 2, cap_points);
  for (int i = 0; i < 2 * n; ++i) xy[i] = t->det[i];
  return (int)t->det.size() / 2;
}

int mpe_tracker_get_distorted_centers(mpe_tracker* t, float* xy, int cap_points) {  // distorted_detection_centers_
  if (!t || (!xy && cap_points > 0)) return MPE_ERR_ARG;
  const int n = std::min<int>((int)t->det_dist.size() / 2, cap_points);
  for (int i = 0; i < 2 * n; ++i) xy[i] = t->det_dist[i];
  return (int)t->det_dist.size() / 2;
}

// ---- the trackers of a rig: one body seen by several cameras -----------------------------------------
// (the joint refinement itself is mpe_rig_optimise_pose_batch, mpe_rig.cpp; here only what reads or sets tracker state)
static Mat4 mat4_from(const double* m) {
  Mat4 r;
  std::memcpy(r.a, m, sizeof(r.a));
  return r;
}

// what mpe_rig_fuse_trackers and mpe_rig_track_trackers refuse before any device work (args_ok: their other pointers)
static int rig_trackers_refused(mpe_tracker* const* ts, int n, bool args_ok) {
  if (!ts || n < 1 || !ts[0]) return MPE_ERR_ARG;
  mpe_handle* h = ts[0]->h;
  if (n > MPE_RIG_MAX_CAMERAS) {
    mpe_host::set_error(h, "n outside 1 .. MPE_RIG_MAX_CAMERAS");
    return MPE_ERR_ARG;
  }
  if (!args_ok) {
    mpe_host::set_error(h, "bad argument");
    return MPE_ERR_ARG;
  }
  for (int i = 0; i < n; ++i) {
    if (!ts[i]) {
      mpe_host::set_error(h, "bad argument");
      return MPE_ERR_ARG;
    }
    if (ts[i]->h != h) {
      mpe_host::set_error(h, "the trackers of a rig must be on one handle");
      return MPE_ERR_ARG;
    }
    for (int j = 0; j < i; ++j)
      if (ts[j] == ts[i]) {
        mpe_host::set_error(h, "a tracker is given twice");
        return MPE_ERR_ARG;
      }
    if (ts[i]->markers != ts[0]->markers) {
      mpe_host::set_error(h, "the trackers of a rig must share one marker set (one body)");
      return MPE_ERR_ARG;
    }
  }
  return MPE_OK;
}

int mpe_rig_fuse_trackers(mpe_tracker* const* ts, int n, const double* T_cam_rig, const int* updated, mpe_result* rig_out,
                          int* rows_per_camera) {
  if (const int refused = rig_trackers_refused(ts, n, T_cam_rig && rig_out)) return refused;
  mpe_handle* h = ts[0]->h;
  std::vector<mpe_rig_camera> cams((size_t)n);
  std::vector<int> row_cam;
  std::vector<double> xyz, uv;
  int first = -1;
  for (int i = 0; i < n; ++i) {
    const mpe_tracker* t = ts[i];
    std::memcpy(cams[(size_t)i].K, t->K, sizeof(t->K));
    std::memcpy(cams[(size_t)i].T_cam_rig, T_cam_rig + 16 * (size_t)i, 16 * sizeof(double));
    int rows = 0;
    if (!updated || updated[i]) {
      const int n_m = n_markers(t), n_d = (int)t->det.size() / 2;
      for (size_t r = 0; r + 1 < t->corr.size() && rows < MPE_MAX_MARKERS; r += 2) {
        const int m = (int)t->corr[r], d = (int)t->corr[r + 1];
        if (m < 1 || m > n_m || d < 1 || d > n_d) continue;
        row_cam.push_back(i);
        xyz.insert(xyz.end(), &t->markers[3 * (size_t)(m - 1)], &t->markers[3 * (size_t)(m - 1)] + 3);
        uv.push_back(t->det[2 * (size_t)(d - 1)]);
        uv.push_back(t->det[2 * (size_t)(d - 1) + 1]);
        ++rows;
      }
      if (rows > 0 && first < 0) first = i;
    }
    if (rows_per_camera) rows_per_camera[i] = rows;
  }
  if (first < 0) {
    std::memset(rig_out, 0, sizeof(*rig_out));
    for (int i = 0; i < 16; i += 5) rig_out->T[i] = 1.0;
    rig_out->status = MPE_FRAME_NO_POSE;
    return 0;
  }
  const Mat4 T0 = matmul(inverse(mat4_from(cams[(size_t)first].T_cam_rig)), ts[first]->predicted);
  const int row_begin[2] = {0, (int)row_cam.size()};
  const int rc = mpe_rig_optimise_pose_batch(h, cams.data(), n, row_begin, row_cam.data(), xyz.data(), uv.data(), 1,
                                             &T0.a[0][0], rig_out);
  if (rc != MPE_OK) return rc;
  return rig_out->status == MPE_FRAME_POSE ? 1 : 0;
}

int mpe_rig_track_trackers(mpe_tracker* const* ts, int n, const double* T_cam_rig, const double rig_pred_pose[16],
                           const mpe_rig_track_options* options, mpe_result* rig_out, uint32_t* match_out,
                           mpe_rig_track_info* info_out) {
  if (const int refused = rig_trackers_refused(ts, n, T_cam_rig && rig_pred_pose && rig_out)) return refused;
  mpe_handle* h = ts[0]->h;
  // every tracker's image points of the frame, updated or not (BatchCtx::advance: those of the whole-image retry when
  // the ROI held fewer than four, those of the ROI when the retry found none)
  std::vector<mpe_rig_camera> cams((size_t)n);
  std::vector<int> det_begin((size_t)n + 1, 0);
  std::vector<double> det_xy, tol_match((size_t)n), tol_accept((size_t)n);
  for (int i = 0; i < n; ++i) {
    const mpe_tracker* t = ts[i];
    std::memcpy(cams[(size_t)i].K, t->K, sizeof(t->K));
    std::memcpy(cams[(size_t)i].T_cam_rig, T_cam_rig + 16 * (size_t)i, 16 * sizeof(double));
    det_xy.insert(det_xy.end(), t->det.begin(), t->det.end());
    det_begin[(size_t)i + 1] = (int)det_xy.size() / 2;
    tol_match[(size_t)i] = t->p.nearest_neighbour_pixel_tolerance;
    tol_accept[(size_t)i] = t->p.back_projection_pixel_tolerance;
  }
  const int rc = mpe_rig_track_batch(h, cams.data(), n, ts[0]->markers.data(), n_markers(ts[0]), det_begin.data(),
                                     det_xy.data(), tol_match.data(), tol_accept.data(), 1, rig_pred_pose, options, rig_out,
                                     match_out, info_out);
  if (rc != MPE_OK) return rc;
  return rig_out->status == MPE_FRAME_POSE ? 1 : 0;
}

int mpe_rig_init_trackers(mpe_tracker* const* ts, int n, const double* T_cam_rig, const mpe_rig_init_options* options,
                          mpe_result* rig_out, uint32_t* match_out, mpe_rig_init_info* info_out) {
  if (const int refused = rig_trackers_refused(ts, n, T_cam_rig && rig_out)) return refused;
  mpe_handle* h = ts[0]->h;
  // every tracker's image points of the frame, as mpe_rig_track_trackers takes them; initialise() votes with the
  // back-projection tolerance, and so does this
  std::vector<mpe_rig_camera> cams((size_t)n);
  std::vector<int> det_begin((size_t)n + 1, 0);
  std::vector<double> det_xy, tol((size_t)n);
  for (int i = 0; i < n; ++i) {
    const mpe_tracker* t = ts[i];
    std::memcpy(cams[(size_t)i].K, t->K, sizeof(t->K));
    std::memcpy(cams[(size_t)i].T_cam_rig, T_cam_rig + 16 * (size_t)i, 16 * sizeof(double));
    det_xy.insert(det_xy.end(), t->det.begin(), t->det.end());
    det_begin[(size_t)i + 1] = (int)det_xy.size() / 2;
    tol[(size_t)i] = t->p.back_projection_pixel_tolerance;
  }
  const int rc = mpe_rig_init_batch(h, cams.data(), n, ts[0]->markers.data(), n_markers(ts[0]), det_begin.data(), det_xy.data(),
                                    tol.data(), tol.data(), 1, options, rig_out, match_out, info_out);
  if (rc != MPE_OK) return rc;
  return rig_out->status == MPE_FRAME_POSE ? 1 : 0;
}

int mpe_rig_init_bodies_trackers(mpe_tracker* const* ts, int n_bodies, int n_cameras, const double* T_cam_rig, const int* find,
                                 const int* updated, double claim_radius_px, mpe_result* rig_out, uint32_t* match_out,
                                 mpe_rig_init_info* info_out, int8_t* owner_out) {
  if (!ts || n_bodies < 1 || n_cameras < 1 || !ts[0]) return MPE_ERR_ARG;
  mpe_handle* h = ts[0]->h;
  if (n_bodies > MPE_MAX_BODIES) {
    mpe_host::set_error(h, "n_bodies outside 1 .. MPE_MAX_BODIES");
    return MPE_ERR_ARG;
  }
  const bool args_ok = (T_cam_rig || n_cameras == 1) && rig_out;
  for (int b = 0; b < n_bodies; ++b) {
    if (const int refused = rig_trackers_refused(ts + (size_t)b * n_cameras, n_cameras, args_ok)) return refused;
    if (ts[(size_t)b * n_cameras]->h != h) {
      mpe_host::set_error(h, "the trackers of all bodies must be on one handle");
      return MPE_ERR_ARG;
    }
    for (int c = 0; c < n_cameras; ++c) {
      const mpe_tracker* t = ts[(size_t)b * n_cameras + c];
      for (size_t k = 0; k < (size_t)b * n_cameras; ++k)
        if (ts[k] == t) {
          mpe_host::set_error(h, "a tracker is given twice");
          return MPE_ERR_ARG;
        }
      // (one camera: the claims compare tracker [b][c]'s undistorted points with the list of tracker [b0][c])
      if (std::memcmp(t->K, ts[c]->K, sizeof(t->K)) != 0 || t->D != ts[c]->D) {
        mpe_host::set_error(h, "the trackers of one camera must share its K and D");
        return MPE_ERR_ARG;
      }
    }
  }
  if (!(claim_radius_px >= 0) || !std::isfinite(claim_radius_px)) {
    mpe_host::set_error(h, "claim_radius_px must be finite and >= 0");
    return MPE_ERR_ARG;
  }
  int b0 = -1;
  for (int b = 0; b < n_bodies && b0 < 0; ++b)
    if (!find || find[b]) b0 = b;
  if (b0 < 0) {  // nobody is asked for: every record "not asked", nothing submitted
    for (int b = 0; b < n_bodies; ++b) {
      std::memset(&rig_out[b], 0, sizeof(mpe_result));
      for (int i = 0; i < 16; i += 5) rig_out[b].T[i] = 1.0;
      rig_out[b].status = MPE_FRAME_NO_POSE;
      if (info_out) {
        std::memset(&info_out[b], 0, sizeof(mpe_rig_init_info));
        info_out[b].reason = 7;
      }
    }
    if (match_out) std::memset(match_out, 0, (size_t)n_bodies * n_cameras * MPE_MAX_MARKERS * sizeof(uint32_t));
    return MPE_OK;
  }
  // camera c's list: the image points of the first searched body's tracker of that camera (as mpe_rig_init_trackers takes
  // them), its back-projection tolerance for the vote and the accept test
  std::vector<mpe_rig_camera> cams((size_t)n_cameras);
  std::vector<int> det_begin((size_t)n_cameras + 1, 0);
  std::vector<double> det_xy, tol((size_t)n_cameras);
  for (int c = 0; c < n_cameras; ++c) {
    const mpe_tracker* t = ts[(size_t)b0 * n_cameras + c];
    std::memcpy(cams[(size_t)c].K, t->K, sizeof(t->K));
    if (T_cam_rig) {
      std::memcpy(cams[(size_t)c].T_cam_rig, T_cam_rig + 16 * (size_t)c, 16 * sizeof(double));
    } else {
      for (int i = 0; i < 16; ++i) cams[(size_t)c].T_cam_rig[i] = (i % 5 == 0) ? 1.0 : 0.0;
    }
    det_xy.insert(det_xy.end(), t->det.begin(), t->det.end());
    det_begin[(size_t)c + 1] = (int)det_xy.size() / 2;
    tol[(size_t)c] = t->p.back_projection_pixel_tolerance;
  }
  // claims at entry: the points the tracked bodies' correspondence rows name, each with its radius (a tracked body's
  // points come from its ROI detection, the list from a whole-image one).  Plain double: two products and one sum.
  std::vector<uint8_t> claimed(det_xy.size() / 2, 0), asked((size_t)n_bodies, 0);
  const double r2 = claim_radius_px * claim_radius_px;
  for (int b = 0; b < n_bodies; ++b) {
    asked[(size_t)b] = (!find || find[b]) ? 1 : 0;
    if (asked[(size_t)b]) continue;
    for (int c = 0; c < n_cameras; ++c) {
      if (updated && !updated[(size_t)b * n_cameras + c]) continue;
      const mpe_tracker* t = ts[(size_t)b * n_cameras + c];
      const int n_m = n_markers(t), n_d = (int)t->det.size() / 2;
      for (size_t r = 0; r + 1 < t->corr.size(); r += 2) {
        const int m = (int)t->corr[r], d = (int)t->corr[r + 1];
        if (m < 1 || m > n_m || d < 1 || d > n_d) continue;
        const double px = t->det[2 * (size_t)(d - 1)], py = t->det[2 * (size_t)(d - 1) + 1];
        for (int q = det_begin[(size_t)c]; q < det_begin[(size_t)c + 1]; ++q) {
          const double dx = det_xy[2 * (size_t)q] - px, dy = det_xy[2 * (size_t)q + 1] - py;
          const double xx = dx * dx, yy = dy * dy;
          if (xx + yy <= r2) claimed[(size_t)q] = 1;
        }
      }
    }
  }
  std::vector<mpe_rig_body> bodies((size_t)n_bodies);
  for (int b = 0; b < n_bodies; ++b) {
    const mpe_tracker* t = ts[(size_t)b * n_cameras];
    bodies[(size_t)b].markers_xyz = t->markers.data();
    bodies[(size_t)b].n_markers = n_markers(t);
    bodies[(size_t)b].options = nullptr;
  }
  const int rc = mpe_rig_init_bodies_batch(h, cams.data(), n_cameras, bodies.data(), n_bodies, det_begin.data(), det_xy.data(),
                                           claimed.data(), asked.data(), tol.data(), tol.data(), 1, rig_out, match_out, info_out,
                                           owner_out);
  if (rc != MPE_OK) return rc;
  int found = 0;
  for (int b = 0; b < n_bodies; ++b) found += rig_out[b].status == MPE_FRAME_POSE ? 1 : 0;
  return found;
}

int mpe_rig_seed_trackers(mpe_tracker* const* ts, int n, const double* T_cam_rig, const int* seed, const double rig_pose[16],
                          double time, const double* rig_prev_pose, double prev_time) {
  if (!ts || n < 1 || n > MPE_RIG_MAX_CAMERAS || !T_cam_rig || !seed || !rig_pose) return MPE_ERR_ARG;
  for (int i = 0; i < n; ++i)
    if (!ts[i]) return MPE_ERR_ARG;
  for (int i = 0; i < n; ++i) {
    if (!seed[i]) continue;
    mpe_tracker* t = ts[i];
    const Mat4 E = mat4_from(T_cam_rig + 16 * (size_t)i);
    t->current = t->predicted = matmul(E, mat4_from(rig_pose));
    t->t_current = time;
    if (rig_prev_pose) {
      t->previous = matmul(E, mat4_from(rig_prev_pose));
      t->t_previous = prev_time;
      t->it_since_initialized = 2;
    } else {
      t->it_since_initialized = 1;
    }
  }
  return MPE_OK;
}

// ---- N trackers in lock step -----------------------------------------------------------------------
// The state machine of estimateBodyPose per stream, with the device steps of all streams that are at the same
// point batched into one submission: DETECT = findLeds in the stream's ROI (+ nearest-neighbour correspondences,
// validation and refinement when tracking), BRUTE = initialise() + optimisePose on the stream's detections.
// A single stream (mpe_tracker_estimate, mpe_tracker_run_sequence) is a group of one.
// A frame is processed in three parts so that a caller can overlap the host work of one group of streams with the
// device work of another: begin (per-stream prediction / ROI), the first DETECT submission (asynchronous), and
// finish (collect it, then whatever else the streams need — second size class, whole-image retries,
// re-initialisations — synchronously, until every stream is done).
}  // extern "C"

namespace {
// (OP_DETECT_WIDE: the stream's detection said MPE_FRAME_TOO_MANY_DETECTIONS and its tracker has the wide switch on —
//  the same detection again through mpe_track_step_batch_wide)
enum BatchOp { OP_DETECT, OP_BRUTE, OP_DONE, OP_DETECT_WIDE };
struct BatchLane {
  BatchOp op = OP_DONE;
  bool tracking = false;  // false: uninitialised branch (detection only, then brute force)
  unsigned num_loops = 0;
  int error = 0;          // per-stream capacity status (< 0) that ended this stream's frame
};

bool same_camera_markers_params(const mpe_tracker* a, const mpe_tracker* b) {
  return a->markers == b->markers && a->D == b->D && !std::memcmp(a->K, b->K, sizeof(a->K)) &&
         !std::memcmp(&a->p, &b->p, sizeof(mpe_params));
}
bool same_setup(const mpe_tracker* a, const mpe_tracker* b) { return a->h == b->h && same_camera_markers_params(a, b); }

struct BatchCtx {
  mpe_tracker* const* ts = nullptr;
  int n = 0;
  const uint8_t* const* imgs = nullptr;
  mpe_handle* h = nullptr;
  std::vector<BatchLane> L;
  std::vector<int> pend;  // lanes of the submitted, not yet collected DETECT batch
  std::vector<mpe_track_item> items;
  std::vector<mpe_detections> dets;
  std::vector<uint32_t> corr;
  std::vector<mpe_result> res;
  std::vector<mpe_detections_wide> wdets;  // records of a wide DETECT call
  // the lanes' set-ups — camera, markers, parameters — as mpe_track_setup entries pointing into the first tracker of
  // each set-up (a uniform group has one), and the set-up of every lane.  mixed (the *_mixed entries) admits lanes of
  // different set-ups on one handle; otherwise every lane must have the first one's.
  bool mixed = false;
  bool frames_on_device = false;  // imgs are device pointers (the *_device entries): the device-frame submission
  std::vector<mpe_track_setup> setups;
  std::vector<int> lane_setup, item_setup;
  // the lanes' image formats — rows, cols, stride in source bytes, encoding —, checked by the entry: formats = the
  // distinct ones (a uniform entry has one), lane_format the index of every lane's among them; item_format that of
  // the gathered items, one_format: they all share item_format[0]
  std::vector<mpe_image_format> formats;
  std::vector<int> lane_format, item_format;
  bool one_format = true;

  // lane i's images are of f[i]
  void set_formats(const mpe_image_format* f) {
    formats.clear();
    lane_format.assign((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
      size_t k = 0;
      while (k < formats.size() && !same_image_format(formats[k], f[i])) ++k;
      if (k == formats.size()) formats.push_back(f[i]);
      lane_format[(size_t)i] = (int)k;
    }
  }
  const mpe_image_format& format_of(int i) const { return formats[(size_t)lane_format[(size_t)i]]; }

  int validate(mpe_tracker* const* ts_, int n_, bool mixed_ = false) {
    ts = ts_;
    n = n_;
    mixed = mixed_;
    for (int i = 0; i < n; ++i) {
      if (!ts[i]) return MPE_ERR_ARG;
      if (mixed ? ts[i]->h != ts[0]->h : !same_setup(ts[0], ts[i]))
        return MPE_ERR_ARG;  // one handle (and, uniform, one camera model, marker set, parameter set)
      for (int j = 0; j < i; ++j)
        if (ts[j] == ts[i]) return MPE_ERR_ARG;
    }
    setups.clear();
    lane_setup.assign((size_t)n, 0);
    std::vector<int> first;  // first lane of every set-up
    for (int i = 0; i < n; ++i) {
      size_t s = 0;
      while (s < first.size() && !same_camera_markers_params(ts[first[s]], ts[i])) ++s;
      if (s == first.size()) {
        const mpe_tracker* t = ts[i];
        first.push_back(i);
        setups.push_back(mpe_track_setup{&t->p, t->K, t->D.empty() ? nullptr : t->D.data(), (int)t->D.size(),
                                         t->markers.data(), n_markers(t)});
      }
      lane_setup[(size_t)i] = (int)s;
    }
    h = ts[0]->h;
    L.assign((size_t)n, BatchLane());
    return MPE_OK;
  }

  // begin of frame: pose_estimator.cpp:62-72 / 98-103 (predictWithROI)
  void begin(const uint8_t* const* imgs_, const double* times) {
    imgs = imgs_;
    for (int i = 0; i < n; ++i) {
      mpe_tracker* t = ts[i];
      const mpe_image_format& f = format_of(i);
      L[(size_t)i] = BatchLane();
      t->pose_updated = false;
      t->used_bruteforce = false;
      // (correspondences_ is a member of the reference object: it keeps its last value when a frame has too few
      //  detections, getCorrespondences() then returns the stale rows — same here)
      t->det.clear();
      t->t_predicted = times[i];
      if (t->it_since_initialized < 1) {
        t->roi[0] = t->roi[1] = 0;
        t->roi[2] = f.cols;
        t->roi[3] = f.rows;
        L[(size_t)i].tracking = false;
      } else {
        if (t->it_since_initialized >= 2)
          t->predicted = predict_pose(t->current, t->previous, t->t_current, t->t_previous, t->t_predicted);
        for (int k = 0; k < n_markers(t); ++k)
          project(t, t->predicted, &t->markers[3 * k], t->predicted_px[2 * k], t->predicted_px[2 * k + 1]);
        determine_roi(t, f.rows, f.cols);
        L[(size_t)i].tracking = true;
      }
      L[(size_t)i].op = OP_DETECT;
    }
  }

  bool is_big(int i) const {
    return (long long)ts[i]->roi[2] * ts[i]->roi[3] * 4 > (long long)format_of(i).rows * format_of(i).cols;
  }

  // the lanes at `op` (of size class `big`; < 0: both — of format `fmt`; < 0: all) as items of a lock-step submission;
  // pend = those lanes
  void gather_items(BatchOp op, int big, int fmt = -1) {
    items.clear();
    item_setup.clear();
    item_format.clear();
    pend.clear();
    one_format = true;
    for (int i = 0; i < n; ++i) {
      if (L[(size_t)i].op != op || (big >= 0 && (int)is_big(i) != big)) continue;
      if (fmt >= 0 && lane_format[(size_t)i] != fmt) continue;
      item_format.push_back(lane_format[(size_t)i]);
      one_format = one_format && item_format.back() == item_format[0];
      const mpe_tracker* t = ts[i];
      mpe_track_item it;
      it.img = imgs[i];
      it.roi_x = t->roi[0];
      it.roi_y = t->roi[1];
      it.roi_w = t->roi[2];
      it.roi_h = t->roi[3];
      it.predicted_px = L[(size_t)i].tracking ? t->predicted_px.data() : nullptr;
      items.push_back(it);
      item_setup.push_back(lane_setup[(size_t)i]);
      pend.push_back(i);
    }
  }
  // submit the DETECT lanes of one size class (two classes, so that a few whole-image retries do not inflate every
  // ROI slot of the batch); returns the number of lanes submitted or < 0
  int submit_detect(int big) {
    gather_items(OP_DETECT, big);
    if (items.empty()) return 0;
    // items of one format (always so in a uniform group): that format alone, as its own entry would submit it — the
    // gather of one format is the faster kernel; else the group's table and every item's index into it
    const mpe_image_format* f = one_format ? &formats[(size_t)item_format[0]] : formats.data();
    const SlotPixels px = {frames_on_device, one_format ? nullptr : item_format.data(), f, one_format ? 1 : (int)formats.size()};
    const int rc = submit_tracked(h, items.data(), item_setup.data(), (int)items.size(), setups.data(), (int)setups.size(), px,
                                  false);
    if (rc != MPE_OK) {
      pend.clear();
      return rc;
    }
    return (int)items.size();
  }

  // collect the submitted DETECT batch and advance its lanes
  int collect_detect() {
    if (pend.empty()) return MPE_OK;
    const int m = (int)pend.size();
    dets.resize((size_t)m);
    corr.resize((size_t)m * 2 * MPE_MAX_MARKERS);
    res.resize((size_t)m);
    const int rc = mpe_track_step_batch_collect(h, dets.data(), corr.data(), res.data());
    if (rc != MPE_OK) return rc;
    for (int k = 0; k < m; ++k) {
      const mpe_detections& d = dets[(size_t)k];
      advance(pend[(size_t)k], d.n, d.status, d.undist_xy, d.dist_xy, res[(size_t)k], &corr[(size_t)k * 2 * MPE_MAX_MARKERS],
              false);
    }
    pend.clear();
    return MPE_OK;
  }

  // lane i behind its detection record (narrow or wide: n_det points, status) with the result and rows the device
  // made from it
  void advance(int i, int n_det, int status, const double* undist_xy, const float* dist_xy, const mpe_result& r,
               const uint32_t* rows_md, bool from_wide) {
    mpe_tracker* t = ts[i];
    BatchLane& ln = L[(size_t)i];
    const bool go_wide = t->wide_frames && !from_wide;
    if (status != 0) {  // device capacity exceeded on this stream's frame
      if (go_wide && status == MPE_FRAME_TOO_MANY_DETECTIONS) {
        ln.op = OP_DETECT_WIDE;
        return;
      }
      ln.error = status;
      ln.op = OP_DONE;
      return;
    }
    if (go_wide && r.status == MPE_FRAME_TOO_MANY_DETECTIONS) {  // (the code on the result alone)
      ln.op = OP_DETECT_WIDE;
      return;
    }
    t->det_dist.assign(dist_xy, dist_xy + 2 * n_det);
    if (n_det > 0) t->det.assign(undist_xy, undist_xy + 2 * n_det);  // kept when nothing was found
    if (!ln.tracking) {  // pose_estimator.cpp:80-91
      ln.op = (t->det.size() / 2 >= 4) ? OP_BRUTE : OP_DONE;
      return;
    }
    ln.num_loops++;  // pose_estimator.cpp:105-144
    if (t->det.size() / 2 >= 4) {
      // (>= 4 detections can only come from this very detection: the device already ran findCorrespondences +
      //  checkCorrespondences + optimisePose on them)
      if (r.status < 0) {
        ln.error = r.status;
        ln.op = OP_DONE;
        return;
      }
      t->n_corr = r.n_corr;
      t->corr.assign(rows_md, rows_md + 2 * r.n_corr);
      if (r.status == MPE_FRAME_POSE) {
        take_result(t, r);
        ln.op = OP_DONE;
      } else {
        ln.op = OP_BRUTE;  // reinitialise if the correspondences were not valid
      }
    } else if (ln.num_loops < 2) {  // too few LEDs in the ROI: search the whole image once
      t->roi[0] = t->roi[1] = 0;
      t->roi[2] = format_of(i).cols;
      t->roi[3] = format_of(i).rows;
      ln.op = OP_DETECT;
    } else {
      ln.op = OP_DONE;
    }
  }

  // the OP_DETECT_WIDE lanes through mpe_track_step_batch_wide (synchronous), one call per distinct format that has
  // such lanes, advanced as collect_detect advances the narrow ones
  int detect_wide() {
    for (size_t fi = 0; fi < formats.size(); ++fi) {
      gather_items(OP_DETECT_WIDE, -1, (int)fi);
      if (items.empty()) continue;
      const int m = (int)items.size();
      wdets.resize((size_t)m);
      corr.resize((size_t)m * 2 * MPE_MAX_MARKERS);
      res.resize((size_t)m);
      const mpe_image_format& f = formats[fi];
      const int rc = mpe_track_step_batch_wide(h, items.data(), item_setup.data(), m, f.rows, f.cols, f.stride_bytes,
                                               frames_on_device ? 1 : 0, f.encoding, f.src_big_endian, setups.data(),
                                               (int)setups.size(), wdets.data(), corr.data(), res.data());
      if (rc != MPE_OK) {
        pend.clear();
        return rc;
      }
      for (int k = 0; k < m; ++k) {
        const mpe_detections_wide& d = wdets[(size_t)k];
        advance(pend[(size_t)k], d.n, d.status, d.undist_xy, d.dist_xy, res[(size_t)k], &corr[(size_t)k * 2 * MPE_MAX_MARKERS],
                true);
      }
      pend.clear();
    }
    return MPE_OK;
  }

  // the OP_BRUTE lanes that hold more than MPE_MAX_DETECTIONS points: mpe_solve_bruteforce_batch_wide, one call per
  // set-up that has such lanes.  Under vote_arith 2 (no strict form) such a lane keeps MPE_FRAME_TOO_MANY_DETECTIONS
  // and the other streams go on.
  int brute_wide() {
    for (size_t s = 0; s < setups.size(); ++s) {
      std::vector<int> idx;
      for (int i = 0; i < n; ++i)
        if (L[(size_t)i].op == OP_BRUTE && lane_setup[(size_t)i] == (int)s && ts[i]->det.size() / 2 > (size_t)MPE_MAX_DETECTIONS)
          idx.push_back(i);
      if (idx.empty()) continue;
      const int m = (int)idx.size();
      const mpe_tracker* t0 = ts[idx[0]];  // (the set-up of these lanes)
      int arith = 0;
      (void)mpe_get_option(h, "vote_arith", &arith);
      if (arith == 2 || n_markers(t0) < 1) {
        for (int i : idx) {
          ts[i]->used_bruteforce = true;
          L[(size_t)i].op = OP_DONE;
          if (arith == 2) L[(size_t)i].error = MPE_FRAME_TOO_MANY_DETECTIONS;
        }
        continue;
      }
      std::vector<double> det_xy((size_t)m * 2 * MPE_WIDE_DETECTIONS, 0.0);
      std::vector<int> nd((size_t)m);
      for (int k = 0; k < m; ++k) {
        const mpe_tracker* t = ts[idx[(size_t)k]];
        nd[(size_t)k] = (int)t->det.size() / 2;
        std::memcpy(&det_xy[(size_t)k * 2 * MPE_WIDE_DETECTIONS], t->det.data(), t->det.size() * sizeof(double));
      }
      const size_t hw = (size_t)MPE_WIDE_DETECTIONS * MPE_MAX_MARKERS;
      res.resize((size_t)m);
      std::vector<uint32_t> hist((size_t)m * hw), bc((size_t)m * 2 * MPE_MAX_MARKERS);
      const int rc = mpe_solve_bruteforce_batch_wide(h, det_xy.data(), nd.data(), m, t0->markers.data(), n_markers(t0), t0->K,
                                                     &t0->p, res.data(), hist.data(), bc.data());
      if (rc != MPE_OK) return rc;
      for (int k = 0; k < m; ++k) {
        const int i = idx[(size_t)k];
        mpe_tracker* t = ts[i];
        const mpe_result& r = res[(size_t)k];
        t->used_bruteforce = true;
        L[(size_t)i].op = OP_DONE;
        if (r.status < 0) {
          L[(size_t)i].error = r.status;
          continue;
        }
        bool any_vote = false;  // initialise() keeps correspondences_ when the histogram is empty (:704-719)
        for (size_t q = 0; q < hw; ++q) any_vote |= hist[(size_t)k * hw + q] != 0;
        if (any_vote) {
          t->n_corr = r.n_corr;
          t->corr.assign(bc.begin() + (size_t)k * 2 * MPE_MAX_MARKERS, bc.begin() + (size_t)k * 2 * MPE_MAX_MARKERS + 2 * r.n_corr);
        }
        if (r.status == MPE_FRAME_POSE) take_result(t, r);
      }
    }
    return MPE_OK;
  }

  // brute-force (re-)initialisations requested so far, in ONE submission: the lanes of one set-up through
  // mpe_solve_bruteforce_batch, the lanes of two or more set-ups through mpe_solve_bruteforce_batch_setups (with a
  // set-up without markers among them: one call per set-up, as it was)
  int brute() {
    for (int i = 0; i < n; ++i)  // (more than MPE_MAX_DETECTIONS points only behind a wide detection)
      if (L[(size_t)i].op == OP_BRUTE && ts[i]->det.size() / 2 > (size_t)MPE_MAX_DETECTIONS) {
        const int rc = brute_wide();
        if (rc != MPE_OK) return rc;
        break;
      }
    int n_with = 0;
    bool all_have_markers = true;  // (the _setups entry refuses a set-up without markers; alone it just finds no pose)
    std::vector<char> has(setups.size(), 0);
    for (int i = 0; i < n; ++i) {
      const size_t s = (size_t)lane_setup[(size_t)i];
      if (L[(size_t)i].op != OP_BRUTE || has[s]) continue;
      has[s] = 1;
      ++n_with;
      all_have_markers = all_have_markers && setups[s].n_markers >= 1;
    }
    if (n_with >= 2 && all_have_markers) return brute_setup(-1);
    for (size_t s = 0; s < setups.size(); ++s) {
      if (!has[s]) continue;
      const int rc = brute_setup((int)s);
      if (rc != MPE_OK) return rc;
    }
    return MPE_OK;
  }
  // setup >= 0: the OP_BRUTE lanes of that set-up; -1: those of every set-up
  int brute_setup(int setup) {
    std::vector<int> idx;
    for (int i = 0; i < n; ++i)
      if (L[(size_t)i].op == OP_BRUTE && (setup < 0 || lane_setup[(size_t)i] == setup)) idx.push_back(i);
    if (idx.empty()) return MPE_OK;
    const int m = (int)idx.size();
    std::vector<double> det_xy((size_t)m * 2 * MPE_MAX_DETECTIONS, 0.0);
    std::vector<int> nd((size_t)m), su((size_t)m), slot_of(setups.size(), -1);
    std::vector<mpe_track_setup> bsetups;
    for (int k = 0; k < m; ++k) {
      const mpe_tracker* t = ts[idx[(size_t)k]];
      nd[(size_t)k] = (int)t->det.size() / 2;
      const int s = lane_setup[(size_t)idx[(size_t)k]];
      if (setup < 0 && slot_of[(size_t)s] < 0) {  // the set-ups that have such lanes, in order of first appearance
        slot_of[(size_t)s] = (int)bsetups.size();
        bsetups.push_back(setups[(size_t)s]);
      }
      su[(size_t)k] = setup < 0 ? slot_of[(size_t)s] : 0;
      std::memcpy(&det_xy[(size_t)k * 2 * MPE_MAX_DETECTIONS], t->det.data(), t->det.size() * sizeof(double));
    }
    res.resize((size_t)m);
    std::vector<uint32_t> hist((size_t)m * MPE_MAX_DETECTIONS * MPE_MAX_MARKERS), bc((size_t)m * 2 * MPE_MAX_MARKERS);
    int rc;
    if (setup >= 0) {
      const mpe_tracker* t0 = ts[idx[0]];  // (the set-up of these lanes)
      rc = mpe_solve_bruteforce_batch(h, det_xy.data(), nd.data(), m, t0->markers.data(), n_markers(t0), t0->K, &t0->p,
                                      res.data(), hist.data(), bc.data());
    } else {
      rc = mpe_solve_bruteforce_batch_setups(h, det_xy.data(), nd.data(), su.data(), m, bsetups.data(), (int)bsetups.size(),
                                             res.data(), hist.data(), bc.data());
    }
    if (rc != MPE_OK) return rc;
    for (int k = 0; k < m; ++k) {
      const int i = idx[(size_t)k];
      mpe_tracker* t = ts[i];
      const mpe_result& r = res[(size_t)k];
      t->used_bruteforce = true;
      L[(size_t)i].op = OP_DONE;
      if (r.status < 0) {
        L[(size_t)i].error = r.status;
        continue;
      }
      bool any_vote = false;  // initialise() keeps correspondences_ when the histogram is empty (:704-719)
      for (size_t q = 0; q < (size_t)MPE_MAX_DETECTIONS * MPE_MAX_MARKERS; ++q)
        any_vote |= hist[(size_t)k * MPE_MAX_DETECTIONS * MPE_MAX_MARKERS + q] != 0;
      if (any_vote) {
        t->n_corr = r.n_corr;
        t->corr.assign(bc.begin() + (size_t)k * 2 * MPE_MAX_MARKERS, bc.begin() + (size_t)k * 2 * MPE_MAX_MARKERS + 2 * r.n_corr);
      }
      if (r.status == MPE_FRAME_POSE) take_result(t, r);
    }
    return MPE_OK;
  }

  // error path: abandon this group's submission if one is in flight, so that its handle accepts the next one (a
  // submission this group did not make — the one that got a call on a busy handle refused — is left alone)
  void cancel() {
    if (pend.empty()) return;
    pend.clear();
    (void)mpe_track_step_batch_cancel(h);
  }

  // first asynchronous submission of a frame: the size class that has lanes (the small one first)
  int submit_first() {
    const int rc = submit_detect(0);
    if (rc != 0) return rc < 0 ? rc : MPE_OK;
    const int rc2 = submit_detect(1);
    return rc2 < 0 ? rc2 : MPE_OK;
  }

  // everything else of the frame, synchronously, until every stream is done
  int finish() {
    int rc = collect_detect();
    if (rc != MPE_OK) return rc;
    for (;;) {
      bool any_detect = false, any_brute = false, any_wide = false;
      for (int i = 0; i < n; ++i) {
        any_detect |= L[(size_t)i].op == OP_DETECT;
        any_brute |= L[(size_t)i].op == OP_BRUTE;
        any_wide |= L[(size_t)i].op == OP_DETECT_WIDE;
      }
      if (!any_detect && !any_brute && !any_wide) break;
      if (any_detect)
        for (int big = 0; big < 2; ++big) {
          const int m = submit_detect(big);
          if (m < 0) return m;
          if (m > 0 && (rc = collect_detect()) != MPE_OK) return rc;
        }
      // (the glare lanes of this iteration, those the detections just collected turned up included, in one call)
      if ((rc = detect_wide()) != MPE_OK) return rc;
      if ((rc = brute()) != MPE_OK) return rc;
    }
    return MPE_OK;
  }

  int outputs(mpe_result* out, size_t out_stride, int* info, size_t info_stride, int* updated) const {
    int n_updated = 0;
    for (int i = 0; i < n; ++i) {
      const mpe_tracker* t = ts[i];
      const int err = L[(size_t)i].error;
      if (out) {
        mpe_result& o = out[(size_t)i * out_stride];
        if (err) {  // a device capacity was exceeded on this stream's frame: as mpe_tracker_run_sequence reports it —
          std::memset(&o, 0, sizeof(o));  // a zeroed record that carries the code
          o.status = err;
        } else {
          std::memcpy(o.T, t->predicted.a, sizeof(o.T));
          std::memcpy(o.cov, t->cov, sizeof(o.cov));
          o.status = t->pose_updated ? MPE_FRAME_POSE : MPE_FRAME_NO_POSE;
          o.n_det = (int)t->det.size() / 2;
          o.n_corr = t->n_corr;
          o.gn_iterations = t->gn_iterations;
        }
      }
      if (info) {
        int* q = info + (size_t)i * info_stride;
        if (err) {
          std::memset(q, 0, 8 * sizeof(int));
        } else {
          for (int k = 0; k < 4; ++k) q[k] = t->roi[k];
          q[4] = (int)t->it_since_initialized;
          q[5] = (int)t->det.size() / 2;
          q[6] = t->n_corr;
          q[7] = t->used_bruteforce ? 1 : 0;
        }
      }
      if (updated) updated[i] = t->pose_updated ? 1 : 0;
      n_updated += t->pose_updated ? 1 : 0;
    }
    return n_updated;
  }
};
}  // namespace

mpe_tracker::~mpe_tracker() { delete solo; }

// one value for each of n lanes: what the uniform entries hand to the per-lane bodies (n as the caller gave it)
template <class T>
static std::vector<T> per_lane(int n, const T& v) {
  return std::vector<T>((size_t)std::max(n, 0), v);
}

extern "C" {

// the formats of n lanes on handle h, before a tracker's state is touched: the codes and texts of the submit entries
static int refuse_formats(mpe_handle* h, const mpe_image_format* formats, int n, bool on_device) {
  for (int i = 0; i < n; ++i) {
    const FormatRefusal no = check_image_format(formats[i], on_device);
    if (no.code == MPE_OK) continue;
    set_error(h, no.msg);
    return no.code;
  }
  return MPE_OK;
}

// one time step of n trackers in lock step; formats[i] is stream i's.  host_as_given: the uniform host entries, whose
// frames are mono8 by signature and whose size was never checked (one that holds no pixels fails the submission's ROI
// check, with that check's text)
static int estimate_batch(mpe_tracker* const* ts, int n, const uint8_t* const* imgs, const mpe_image_format* formats,
                          const double* times, mpe_result* out, int* info, int* updated, bool mixed, bool on_device,
                          bool host_as_given = false) {
  if (!ts || n < 0 || !imgs || !times) return MPE_ERR_ARG;
  if (n == 0) return 0;
  for (int i = 0; i < n; ++i)
    if (!imgs[i]) return MPE_ERR_ARG;
  BatchCtx c;
  int rc = c.validate(ts, n, mixed);
  if (rc != MPE_OK) return rc;
  if (!host_as_given && (rc = refuse_formats(c.h, formats, n, on_device)) != MPE_OK) return rc;
  c.frames_on_device = on_device;
  c.set_formats(formats);
  c.begin(imgs, times);
  if ((rc = c.submit_first()) != MPE_OK || (rc = c.finish()) != MPE_OK) {
    c.cancel();  // (a submission may still be in flight: leave the handle usable)
    return rc;
  }
  return c.outputs(out, 1, info, 8, updated);
}

// one stream: a lock-step group of one
int mpe_tracker_estimate(mpe_tracker* t, const uint8_t* img, int rows, int cols, size_t stride_bytes, double time,
                         mpe_result* out, int info[8]) {
  if (!t || !img) return MPE_ERR_ARG;
  if (!t->solo) t->solo = new BatchCtx();
  BatchCtx& c = *t->solo;
  int rc = c.validate(&t, 1);
  if (rc != MPE_OK) return rc;
  const mpe_image_format f = {rows, cols, stride_bytes, MPE_ENC_MONO8, 0};
  c.set_formats(&f);
  c.begin(&img, &time);
  if ((rc = c.submit_first()) != MPE_OK || (rc = c.finish()) != MPE_OK) {
    c.cancel();
    return rc;
  }
  if (c.L[0].error) {  // a device capacity was exceeded on this frame: its code, out / info untouched
    mpe_host::set_error(t->h, "frame exceeded a device capacity");
    return c.L[0].error;
  }
  return c.outputs(out, 1, info, 8, nullptr);
}

int mpe_tracker_estimate_batch(mpe_tracker* const* ts, int n, const uint8_t* const* imgs, int rows, int cols,
                               size_t stride_bytes, const double* times, mpe_result* out, int* info, int* updated) {
  const std::vector<mpe_image_format> f = per_lane(n, mpe_image_format{rows, cols, stride_bytes, MPE_ENC_MONO8, 0});
  return estimate_batch(ts, n, imgs, f.data(), times, out, info, updated, false, false, true);
}

int mpe_tracker_estimate_batch_mixed(mpe_tracker* const* ts, int n, const uint8_t* const* imgs, int rows, int cols,
                                     size_t stride_bytes, const double* times, mpe_result* out, int* info, int* updated) {
  const std::vector<mpe_image_format> f = per_lane(n, mpe_image_format{rows, cols, stride_bytes, MPE_ENC_MONO8, 0});
  return estimate_batch(ts, n, imgs, f.data(), times, out, info, updated, true, false, true);
}

// the frames in device memory (host array of device pointers); set-ups may be mixed, as in the entry above
int mpe_tracker_estimate_batch_device(mpe_tracker* const* ts, int n, const uint8_t* const* d_imgs, int rows, int cols,
                                      size_t stride_bytes, const double* times, mpe_result* out, int* info, int* updated) {
  const std::vector<mpe_image_format> f = per_lane(n, mpe_image_format{rows, cols, stride_bytes, MPE_ENC_MONO8, 0});
  return estimate_batch(ts, n, d_imgs, f.data(), times, out, info, updated, true, true);
}

// the frames in device memory in the camera's own encoding: the ROI gather decodes them (stride_bytes in source bytes)
int mpe_tracker_estimate_batch_device_encoded(mpe_tracker* const* ts, int n, const uint8_t* const* d_imgs, int rows, int cols,
                                              size_t stride_bytes, int encoding, int src_big_endian, const double* times,
                                              mpe_result* out, int* info, int* updated) {
  const std::vector<mpe_image_format> f = per_lane(n, mpe_image_format{rows, cols, stride_bytes, encoding, src_big_endian});
  return estimate_batch(ts, n, d_imgs, f.data(), times, out, info, updated, true, true);
}

// trackers whose cameras differ in image format (size, stride, encoding): formats[i] is stream i's
int mpe_tracker_estimate_batch_formats(mpe_tracker* const* ts, int n, const uint8_t* const* imgs, int frames_on_device,
                                       const mpe_image_format* formats, const double* times, mpe_result* out, int* info,
                                       int* updated) {
  if (!formats) return MPE_ERR_ARG;
  return estimate_batch(ts, n, imgs, formats, times, out, info, updated, true, frames_on_device != 0);
}

// The lock-step loops of N streams over recorded sequences.  Trackers that live on DIFFERENT handles form groups
// (one group per handle, each with the same camera / marker / parameter set inside the group); the groups are
// pipelined against each other: while the device works on step k of one group, the host collects, advances and
// packs another — the host work of a time step (~3 us per stream) hides behind the device latency (~0.2 ms).
// Stream i's images are of formats[i] and its frames frame_strides[i] bytes apart.
// (mixed: each group may mix cameras, marker sets and parameters — mpe_tracker_run_sequences_batch_mixed_threads)
static int run_sequences_batch(mpe_tracker* const* ts, int n, const uint8_t* const* frames, int n_frames,
                               const mpe_image_format* formats, const size_t* frame_strides, const double* times,
                               mpe_result* out, int* info, int n_threads, bool mixed, bool on_device,
                               bool host_as_given = false) {
  if (!ts || n < 0 || !frames || !times || n_frames < 0 || n_threads < 1) return MPE_ERR_ARG;
  if (n == 0 || n_frames == 0) return 0;
  for (int i = 0; i < n; ++i)
    if (!ts[i] || !frames[i]) return MPE_ERR_ARG;
  // groups by handle, in order of first appearance
  std::vector<mpe_handle*> hs;
  std::vector<std::vector<int> > members;
  for (int i = 0; i < n; ++i) {
    size_t g = 0;
    while (g < hs.size() && hs[g] != ts[i]->h) ++g;
    if (g == hs.size()) {
      hs.push_back(ts[i]->h);
      members.push_back(std::vector<int>());
    }
    members[g].push_back(i);
  }
  const size_t G = hs.size();
  std::vector<BatchCtx> ctx(G);
  std::vector<std::vector<mpe_tracker*> > gts(G);
  std::vector<std::vector<const uint8_t*> > gimgs(G);
  std::vector<std::vector<double> > gtimes(G);
  std::vector<std::vector<mpe_image_format> > gformats(G);
  for (size_t g = 0; g < G; ++g) {
    for (int i : members[g]) gts[g].push_back(ts[i]);
    gimgs[g].resize(members[g].size());
    gtimes[g].resize(members[g].size());
    const int rc = ctx[g].validate(gts[g].data(), (int)gts[g].size(), mixed);
    if (rc != MPE_OK) return rc;
    ctx[g].frames_on_device = on_device;
  }
  for (size_t g = 0; g < G; ++g) {
    for (int i : members[g]) gformats[g].push_back(formats[i]);
    if (host_as_given) continue;  // (as in estimate_batch)
    const int rc = refuse_formats(hs[g], gformats[g].data(), (int)gformats[g].size(), on_device);
    if (rc != MPE_OK) return rc;
  }
  for (size_t g = 0; g < G; ++g) ctx[g].set_formats(gformats[g].data());
  // The groups gs[0..) on the calling thread, pipelined against each other: while the device works on step k of one
  // group, the host collects, advances and packs another.  Groups share nothing (own handle, own trackers, own rows
  // of out / info), so disjoint sets of groups can also run on different host threads.
  auto run_groups_impl = [&](const std::vector<size_t>& gs, long long& updated) -> int {
    std::vector<mpe_result> step_out((size_t)n);
    std::vector<int> step_info((size_t)n * 8);
    auto finish_group = [&](size_t g, int f) -> int {  // complete step f of group g and store its records
      int rc = ctx[g].finish();
      if (rc != MPE_OK) return rc;
      const int m = (int)members[g].size();
      updated += ctx[g].outputs(step_out.data(), 1, step_info.data(), 8, nullptr);
      for (int k = 0; k < m; ++k) {
        const int i = members[g][(size_t)k];
        if (out) out[(size_t)i * n_frames + f] = step_out[(size_t)k];
        if (info) std::memcpy(info + ((size_t)i * n_frames + f) * 8, &step_info[(size_t)k * 8], 8 * sizeof(int));
      }
      return MPE_OK;
    };
    for (int f = 0; f < n_frames; ++f)
      for (size_t g : gs) {
        if (f > 0) {
          const int rc = finish_group(g, f - 1);
          if (rc != MPE_OK) return rc;
        }
        for (size_t k = 0; k < members[g].size(); ++k) {
          gimgs[g][k] = frames[members[g][k]] + (size_t)f * frame_strides[members[g][k]];
          gtimes[g][k] = times[f];
        }
        ctx[g].begin(gimgs[g].data(), gtimes[g].data());
        const int rc = ctx[g].submit_first();
        if (rc != MPE_OK) return rc;
      }
    for (size_t g : gs) {
      const int rc = finish_group(g, n_frames - 1);
      if (rc != MPE_OK) return rc;
    }
    return MPE_OK;
  };
  // on any error every group of the set is drained: the other groups' submissions would otherwise stay un-collected
  // and their handles would refuse every later mpe_track_step / _submit
  auto run_groups = [&](const std::vector<size_t>& gs, long long& updated) -> int {
    const int rc = run_groups_impl(gs, updated);
    if (rc != MPE_OK)
      for (size_t g : gs) ctx[g].cancel();
    return rc;
  };
  const size_t T = std::min<size_t>((size_t)n_threads, G);
  std::vector<std::vector<size_t> > sets(T);
  for (size_t g = 0; g < G; ++g) sets[g % T].push_back(g);
  std::vector<long long> upd(T, 0);
  std::vector<int> rcs(T, MPE_OK);
  if (T <= 1) {
    rcs[0] = run_groups(sets[0], upd[0]);
  } else {
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; ++t) th.emplace_back([&, t]() { rcs[t] = run_groups(sets[t], upd[t]); });
    for (auto& x : th) x.join();
  }
  long long updated = 0;
  for (size_t t = 0; t < T; ++t) {
    if (rcs[t] != MPE_OK) return rcs[t];
    updated += upd[t];
  }
  return (int)std::min<long long>(updated, 0x7fffffff);
}

int mpe_tracker_run_sequences_batch_threads(mpe_tracker* const* ts, int n, const uint8_t* const* frames, int n_frames,
                                            int rows, int cols, size_t stride_bytes, size_t frame_stride_bytes,
                                            const double* times, mpe_result* out, int* info, int n_threads) {
  const std::vector<mpe_image_format> f = per_lane(n, mpe_image_format{rows, cols, stride_bytes, MPE_ENC_MONO8, 0});
  const std::vector<size_t> fs = per_lane(n, frame_stride_bytes);
  return run_sequences_batch(ts, n, frames, n_frames, f.data(), fs.data(), times, out, info, n_threads,
                             false, false, true);
}

int mpe_tracker_run_sequences_batch_mixed_threads(mpe_tracker* const* ts, int n, const uint8_t* const* frames,
                                                  int n_frames, int rows, int cols, size_t stride_bytes,
                                                  size_t frame_stride_bytes, const double* times, mpe_result* out,
                                                  int* info, int n_threads) {
  const std::vector<mpe_image_format> f = per_lane(n, mpe_image_format{rows, cols, stride_bytes, MPE_ENC_MONO8, 0});
  const std::vector<size_t> fs = per_lane(n, frame_stride_bytes);
  return run_sequences_batch(ts, n, frames, n_frames, f.data(), fs.data(), times, out, info, n_threads,
                             true, false, true);
}

// frames[i] = DEVICE pointer to stream i's sequence (host array of device pointers); groups as in the entry above
int mpe_tracker_run_sequences_batch_device_threads(mpe_tracker* const* ts, int n, const uint8_t* const* d_frames,
                                                   int n_frames, int rows, int cols, size_t stride_bytes,
                                                   size_t frame_stride_bytes, const double* times, mpe_result* out,
                                                   int* info, int n_threads) {
  const std::vector<mpe_image_format> f = per_lane(n, mpe_image_format{rows, cols, stride_bytes, MPE_ENC_MONO8, 0});
  const std::vector<size_t> fs = per_lane(n, frame_stride_bytes);
  return run_sequences_batch(ts, n, d_frames, n_frames, f.data(), fs.data(), times, out, info, n_threads,
                             true, true);
}

// ... in the camera's own encoding (stride_bytes and frame_stride_bytes in source bytes)
int mpe_tracker_run_sequences_batch_device_encoded_threads(mpe_tracker* const* ts, int n, const uint8_t* const* d_frames,
                                                           int n_frames, int rows, int cols, size_t stride_bytes,
                                                           size_t frame_stride_bytes, int encoding, int src_big_endian,
                                                           const double* times, mpe_result* out, int* info, int n_threads) {
  const std::vector<mpe_image_format> f = per_lane(n, mpe_image_format{rows, cols, stride_bytes, encoding, src_big_endian});
  const std::vector<size_t> fs = per_lane(n, frame_stride_bytes);
  return run_sequences_batch(ts, n, d_frames, n_frames, f.data(), fs.data(), times, out, info, n_threads,
                             true, true);
}

// ... every stream in an image format of its own
int mpe_tracker_run_sequences_batch_formats_threads(mpe_tracker* const* ts, int n, const uint8_t* const* frames, int n_frames,
                                                    int frames_on_device, const mpe_image_format* formats,
                                                    const size_t* frame_stride_bytes, const double* times, mpe_result* out,
                                                    int* info, int n_threads) {
  if (!formats || !frame_stride_bytes) return MPE_ERR_ARG;
  return run_sequences_batch(ts, n, frames, n_frames, formats, frame_stride_bytes, times, out, info, n_threads, true,
                             frames_on_device != 0);
}

int mpe_tracker_run_sequences_batch(mpe_tracker* const* ts, int n, const uint8_t* const* frames, int n_frames, int rows,
                                    int cols, size_t stride_bytes, size_t frame_stride_bytes, const double* times,
                                    mpe_result* out, int* info) {
  return mpe_tracker_run_sequences_batch_threads(ts, n, frames, n_frames, rows, cols, stride_bytes, frame_stride_bytes,
                                                 times, out, info, 1);
}

// one stream's sequence: the lock-step loop over a group of one (a frame that exceeds a device capacity gets a zeroed
// record that carries the code, and the sequence goes on)
int mpe_tracker_run_sequence(mpe_tracker* t, const uint8_t* frames, int n_frames, int rows, int cols,
                             size_t stride_bytes, size_t frame_stride_bytes, const double* times, mpe_result* out,
                             int* info) {
  if (!t || !frames || !times || n_frames < 0) return MPE_ERR_ARG;
  const mpe_image_format f = {rows, cols, stride_bytes, MPE_ENC_MONO8, 0};
  return run_sequences_batch(&t, 1, &frames, n_frames, &f, &frame_stride_bytes, times, out, info, 1, false, false, true);
}

}  // extern "C"
