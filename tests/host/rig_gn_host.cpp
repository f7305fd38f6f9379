// rig_gn_host.cpp — the logic of k_rig_refine (csrc/mpe_rig_gn.h) compiled for the host (test scaffolding, CPU tier): the
// header as it is, behind the tail helpers of mpe_k3.hip (`struct T34` .. `#define K3_GROUP`, cut out at test time into
// k3_extract.inc as tests/host/geom_host.cpp has them).  A phase of the header runs its 64 lanes one after the other here.
// Two uses: a shared library for tests/test_rig_gn_host.py (host_rig_refine against the numpy witness, host_gauss_newton
// for the one-camera identity), and — with -DRIG_GN_HOST_MAIN — a stand-alone program that tools/host_sanitize.sh and the
// test build under -fsanitize=address,undefined: one camera with the identity extrinsic against k3_gauss_newton bit for
// bit, exact-pixel rigs of 1 .. 16 cameras and 3 .. 256 rows (65 and 256 among them) back to their true pose, and the
// short problems (0 and 2 rows).  Prints "rig_gn_host ok: ..." and returns 0, or says what failed and returns 1.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include <hip/hip_runtime.h>  // (tests/host/stub: the one-lane meaning of the HIP spellings)

#include "../../include/mpe.h"
namespace mpe {
#include "k3_extract.inc"
#include "mpe_rig_gn.h"
}  // namespace mpe
using namespace mpe;

extern "C" void host_rig_refine(const mpe_rig_camera* cams, int n_cam, const int* row_cam, const double* row_xyz,
                                const double* row_uv, int n_rows, const double* T_init, mpe_result* out) {
  RigGnLds* G = new RigGnLds;  // (the kernel's LDS; every byte that is read has been written by a phase before)
  rig_gn_refine(*G, cams, n_cam, row_cam, row_xyz, row_uv, n_rows, T_init, out);
  delete G;
}

// optimisePose as k3b_refine runs it (tests/host/geom_host.cpp): rows = n_c x (marker xyz, detection uv)
extern "C" int host_gauss_newton(const double* rows, int n_c, const double* k4, double* T34_rows, double* cov) {
  T34 T;
  std::memcpy(T.m, T34_rows, sizeof(T.m));
  const int it = k3_gauss_newton(n_c, [&](int j, int k) -> double { return rows[5 * j + k]; }, k4[0], k4[1], k4[2],
                                 k4[3], T, cov);
  std::memcpy(T34_rows, T.m, sizeof(T.m));
  return it;
}

#ifdef RIG_GN_HOST_MAIN
namespace {
int g_failed = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      std::printf("FAILED %s: ", #cond); \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
      ++g_failed;                        \
    }                                    \
  } while (0)

struct M4 {
  double a[16];
};
M4 rigid(std::mt19937& g, double max_angle, double max_shift) {
  std::normal_distribution<double> nd;
  std::uniform_real_distribution<double> ud(0.0, 1.0);
  double ax[3] = {nd(g), nd(g), nd(g)};
  const double nrm = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
  const double th = max_angle * ud(g), s = std::sin(th), c = std::cos(th);
  for (double& v : ax) v /= nrm;
  M4 m;
  const double K[3][3] = {{0, -ax[2], ax[1]}, {ax[2], 0, -ax[0]}, {-ax[1], ax[0], 0}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double k2 = 0;
      for (int k = 0; k < 3; ++k) k2 += K[i][k] * K[k][j];
      m.a[4 * i + j] = (i == j ? 1.0 : 0.0) + s * K[i][j] + (1 - c) * k2;
    }
  for (int i = 0; i < 3; ++i) m.a[4 * i + 3] = max_shift * (2 * ud(g) - 1);
  m.a[12] = m.a[13] = m.a[14] = 0;
  m.a[15] = 1;
  return m;
}
M4 mul(const M4& x, const M4& y) {
  M4 r;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = 0;
      for (int k = 0; k < 4; ++k) s += x.a[4 * i + k] * y.a[4 * k + j];
      r.a[4 * i + j] = s;
    }
  return r;
}
void apply(const M4& T, const double* p, double* q) {
  for (int i = 0; i < 3; ++i) q[i] = T.a[4 * i] * p[0] + T.a[4 * i + 1] * p[1] + T.a[4 * i + 2] * p[2] + T.a[4 * i + 3];
}
}  // namespace

int main() {
  std::mt19937 g(20240607);
  std::uniform_real_distribution<double> ud(0.0, 1.0);
  long n_ident = 0, n_rigs = 0, n_short = 0, rows_most = 0;
  // a body in front of the rig: T_true = a small rotation, 1.5 m down the axis
  auto body_pose = [&]() {
    M4 T = rigid(g, 0.6, 0.2);
    T.a[11] += 1.5;
    return T;
  };
  // ---- one camera, identity extrinsic: k3_gauss_newton's pose, covariance and count
  for (int it = 0; it < 200; ++it) {
    const int n_c = 3 + (int)(g() % 14);  // 3 .. 16 rows
    mpe_rig_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.K[0] = 420 + 20 * ud(g), cam.K[4] = 425 + 20 * ud(g), cam.K[2] = 370 + 10 * ud(g), cam.K[5] = 235 + 10 * ud(g), cam.K[8] = 1;
    for (int i = 0; i < 16; i += 5) cam.T_cam_rig[i] = 1.0;
    const M4 T_true = body_pose();
    std::vector<double> xyz(3 * n_c), uv(2 * n_c), rows5(5 * n_c);
    std::vector<int> rc(n_c, 0);
    for (int j = 0; j < n_c; ++j) {
      for (int k = 0; k < 3; ++k) xyz[3 * j + k] = 0.3 * (2 * ud(g) - 1);
      double q[3];
      apply(T_true, &xyz[3 * j], q);
      uv[2 * j] = cam.K[0] * q[0] / q[2] + cam.K[2] + 0.2 * (2 * ud(g) - 1);
      uv[2 * j + 1] = cam.K[4] * q[1] / q[2] + cam.K[5] + 0.2 * (2 * ud(g) - 1);
      for (int k = 0; k < 3; ++k) rows5[5 * j + k] = xyz[3 * j + k];
      rows5[5 * j + 3] = uv[2 * j];
      rows5[5 * j + 4] = uv[2 * j + 1];
    }
    const M4 T0 = mul(rigid(g, 0.05, 0.01), T_true);
    mpe_result r;
    std::memset(&r, 0xff, sizeof(r));
    host_rig_refine(&cam, 1, rc.data(), xyz.data(), uv.data(), n_c, T0.a, &r);
    double T34_rows[12], cov[36];
    std::memcpy(T34_rows, T0.a, sizeof(T34_rows));
    const double k4[4] = {cam.K[0], cam.K[4], cam.K[2], cam.K[5]};
    const int iters = host_gauss_newton(rows5.data(), n_c, k4, T34_rows, cov);
    CHECK(iters == r.gn_iterations, "problem %d: %d iterations against %d", it, r.gn_iterations, iters);
    CHECK(std::memcmp(T34_rows, r.T, sizeof(T34_rows)) == 0, "problem %d: pose differs", it);
    CHECK(std::memcmp(cov, r.cov, sizeof(cov)) == 0, "problem %d: covariance differs", it);
    CHECK(r.n_corr == n_c && r.n_det == 1 && r.T[15] == 1.0 && r.T[12] == 0.0, "problem %d: record", it);
    ++n_ident;
  }
  // ---- rigs with exact pixels: back to the true pose
  for (int it = 0; it < 120; ++it) {
    // (three distinct markers at least, four for a lone camera: fewer leave the pose open whatever the camera count)
    int n_cam = 1 + (int)(g() % MPE_RIG_MAX_CAMERAS), per = 3 + (int)(g() % (MPE_MAX_MARKERS - 2));
    if (n_cam == 1 && per < 4) per = 4;
    if (it == 0) n_cam = 16, per = 16;  // 256 rows: the cap
    if (it == 1) n_cam = 5, per = 13;   // 65 rows: one more than a wave
    if (it == 2) n_cam = 2, per = 3;
    std::vector<mpe_rig_camera> cams(n_cam);
    std::vector<M4> E(n_cam);
    for (int c = 0; c < n_cam; ++c) {
      std::memset(&cams[c], 0, sizeof(cams[c]));
      cams[c].K[0] = 420 + 20 * ud(g), cams[c].K[4] = 425 + 20 * ud(g), cams[c].K[2] = 370, cams[c].K[5] = 235, cams[c].K[8] = 1;
      E[c] = rigid(g, 0.5, 0.3);
      std::memcpy(cams[c].T_cam_rig, E[c].a, sizeof(E[c].a));
    }
    const M4 T_true = body_pose();
    std::vector<double> mk(3 * MPE_MAX_MARKERS);
    for (double& v : mk) v = 0.3 * (2 * ud(g) - 1);
    std::vector<int> rc;
    std::vector<double> xyz, uv;
    for (int c = 0; c < n_cam; ++c)
      for (int j = 0; j < per; ++j) {
        double X[3], q[3];
        apply(T_true, &mk[3 * j], X);
        apply(E[c], X, q);
        rc.push_back(c);
        xyz.insert(xyz.end(), &mk[3 * j], &mk[3 * j] + 3);
        uv.push_back(cams[c].K[0] * q[0] / q[2] + cams[c].K[2]);
        uv.push_back(cams[c].K[4] * q[1] / q[2] + cams[c].K[5]);
      }
    const int n_rows = (int)rc.size();
    const M4 T0 = mul(rigid(g, 0.05, 0.01), T_true);
    mpe_result r;
    std::memset(&r, 0xff, sizeof(r));
    host_rig_refine(cams.data(), n_cam, rc.data(), xyz.data(), uv.data(), n_rows, T0.a, &r);
    double worst = 0;
    for (int i = 0; i < 16; ++i) worst = std::fmax(worst, std::fabs(r.T[i] - T_true.a[i]));
    CHECK(r.status == MPE_FRAME_POSE && r.n_corr == n_rows && r.n_det == n_cam, "rig %d: status %d rows %d cameras %d", it,
          r.status, r.n_corr, r.n_det);
    CHECK(worst < 1e-9 && r.gn_iterations >= 2 && r.gn_iterations <= 20, "rig %d (%d x %d): %.3g off after %d iterations", it,
          n_cam, per, worst, r.gn_iterations);
    for (int i = 0; i < 6; ++i) CHECK(r.cov[7 * i] > 0, "rig %d: variance %d = %g", it, i, r.cov[7 * i]);
    rows_most = n_rows > rows_most ? n_rows : rows_most;
    ++n_rigs;
  }
  // ---- fewer than three rows: no pose, the start pose handed back, a zero covariance
  for (int n_rows = 0; n_rows < 3; ++n_rows) {
    mpe_rig_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.K[0] = cam.K[4] = 400, cam.K[2] = 370, cam.K[5] = 235, cam.K[8] = 1;
    for (int i = 0; i < 16; i += 5) cam.T_cam_rig[i] = 1.0;
    const M4 T0 = body_pose();
    const int rc[2] = {0, 0};
    const double xyz[6] = {0.1, 0, 0, 0, 0.1, 0}, uv[4] = {380, 240, 370, 250};
    mpe_result r;
    std::memset(&r, 0xff, sizeof(r));
    host_rig_refine(&cam, 1, rc, xyz, uv, n_rows, T0.a, &r);
    CHECK(r.status == MPE_FRAME_NO_POSE && r.gn_iterations == 0 && r.n_corr == n_rows && r.n_det == (n_rows ? 1 : 0), "%d rows: record",
          n_rows);
    CHECK(std::memcmp(r.T, T0.a, sizeof(T0.a)) == 0, "%d rows: the start pose comes back", n_rows);
    for (int i = 0; i < 36; ++i) CHECK(r.cov[i] == 0.0, "%d rows: cov[%d]", n_rows, i);
    ++n_short;
  }
  if (g_failed) {
    std::printf("rig_gn_host: %d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("rig_gn_host ok: %ld one-camera problems bit-equal, %ld rigs (up to %ld rows), %ld short problems\n", n_ident,
              n_rigs, rows_most, n_short);
  return 0;
}
#endif
