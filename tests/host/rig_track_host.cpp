// rig_track_host.cpp — the logic of k_rig_track (csrc/mpe_rig_track.h) compiled for the host (test scaffolding, CPU tier):
// the header as it is, behind mpe_rig_gn.h and the tail helpers of mpe_k3.hip (`struct T34` .. `#define K3_GROUP`, cut out
// at test time into k3_extract.inc as tests/host/rig_gn_host.cpp has them).  A phase runs its 64 lanes one after the other
// here.  Two uses: a shared library for tests/test_rig_track_host.py (host_rig_track against the numpy witness,
// host_rig_refine for the pins), and — with -DRIG_TRACK_HOST_MAIN — a stand-alone program that the test builds plain and
// under -fsanitize=address,undefined: rigs of 1 .. 16 cameras and 4 .. 16 markers with exact pixels among stray
// detections (16 x 16 = 256 pairs, a camera without detections and one with 64 among them) back to their true pose, the
// max_rounds = 1 record against rig_gn_refine over the matched rows bit for bit, and the problems without a pose
// (reasons 1, 2 and 4).  Prints "rig_track_host ok: ..." and returns 0, or says what failed and returns 1.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include <hip/hip_runtime.h>  // (tests/host/stub: the one-lane meaning of the HIP spellings)

#include "../../include/mpe.h"
namespace mpe {
#include "k3_extract.inc"
#include "mpe_rig_gn.h"
#include "mpe_rig_track.h"
}  // namespace mpe
using namespace mpe;

extern "C" void host_rig_track(const mpe_rig_camera* cams, int n_cam, const double* markers, int n_mk, const int* det_begin,
                               const double* det_xy, const double* tol_match, const double* tol_accept, const double* T_pred,
                               int max_rounds, int min_rows, int min_markers, mpe_result* out, uint32_t* match,
                               mpe_rig_track_info* info) {
  RigTrackLds* S = new RigTrackLds;  // (the kernel's LDS; every byte that is read has been written by a phase before)
  rig_track(*S, cams, n_cam, markers, n_mk, det_begin, det_xy, tol_match, tol_accept, T_pred, max_rounds, min_rows,
            min_markers, out, match, info);
  delete S;
}

extern "C" void host_rig_refine(const mpe_rig_camera* cams, int n_cam, const int* row_cam, const double* row_xyz,
                                const double* row_uv, int n_rows, const double* T_init, mpe_result* out) {
  RigGnLds* G = new RigGnLds;
  rig_gn_refine(*G, cams, n_cam, row_cam, row_xyz, row_uv, n_rows, T_init, out);
  delete G;
}

extern "C" int host_rig_track_lds_bytes() { return (int)sizeof(RigTrackLds); }

#ifdef RIG_TRACK_HOST_MAIN
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

struct Problem {
  std::vector<mpe_rig_camera> cams;
  std::vector<double> mk, det, tol_m, tol_a;
  std::vector<int> beg;
  M4 T_true, T_pred;
  int n_cam, n_mk, n_seen_rows;
};
// camera c sees the first seen[c] markers (exact pixels) among stray[c] stray detections far from every LED
Problem make(std::mt19937& g, int n_cam, int n_mk, const std::vector<int>& seen, const std::vector<int>& stray) {
  std::uniform_real_distribution<double> ud(0.0, 1.0);
  Problem P;
  P.n_cam = n_cam, P.n_mk = n_mk, P.n_seen_rows = 0;
  P.cams.resize(n_cam);
  P.mk.resize(3 * n_mk);
  for (double& v : P.mk) v = 0.5 * (2 * ud(g) - 1);
  P.T_true = rigid(g, 0.6, 0.2);
  P.T_true.a[11] += 1.8;
  P.T_pred = mul(rigid(g, 0.001, 0.001), P.T_true);
  P.beg.assign(1, 0);
  for (int c = 0; c < n_cam; ++c) {
    mpe_rig_camera& cam = P.cams[c];
    std::memset(&cam, 0, sizeof(cam));
    cam.K[0] = 420 + 20 * ud(g), cam.K[4] = 425 + 20 * ud(g), cam.K[2] = 370, cam.K[5] = 235, cam.K[8] = 1;
    // (an extrinsic under which the LEDs are 10 px apart at least: the start below moves a pixel by 2 px at the most)
    std::vector<double> led(2 * n_mk);
    for (bool apart = false; !apart;) {
      const M4 E = rigid(g, 0.4, 0.3);
      std::memcpy(cam.T_cam_rig, E.a, sizeof(E.a));
      for (int m = 0; m < n_mk; ++m) {
        double X[3], q[3];
        apply(P.T_true, &P.mk[3 * m], X);
        apply(E, X, q);
        led[2 * m] = cam.K[0] * q[0] / q[2] + cam.K[2];
        led[2 * m + 1] = cam.K[4] * q[1] / q[2] + cam.K[5];
      }
      apart = true;
      for (int m = 0; m < n_mk; ++m)
        for (int k = 0; k < m; ++k) apart = apart && std::hypot(led[2 * m] - led[2 * k], led[2 * m + 1] - led[2 * k + 1]) >= 10.0;
    }
    // the stray detections first, so that a row's detection index is not its marker index
    for (int k = 0; k < stray[c];) {
      const double x = 2000 * ud(g) - 600, y = 1500 * ud(g) - 500;
      bool far = true;
      for (int m = 0; m < n_mk; ++m) far = far && std::hypot(x - led[2 * m], y - led[2 * m + 1]) > 40.0;
      if (!far) continue;
      P.det.push_back(x), P.det.push_back(y);
      ++k;
    }
    for (int m = 0; m < seen[c]; ++m) P.det.push_back(led[2 * m]), P.det.push_back(led[2 * m + 1]);
    P.n_seen_rows += seen[c];
    P.beg.push_back((int)P.det.size() / 2);
  }
  P.tol_m.assign(n_cam, 12.0);
  P.tol_a.assign(n_cam, 3.0);
  return P;
}
struct Answer {
  mpe_result r;
  std::vector<uint32_t> match;
  mpe_rig_track_info info;
};
Answer run(const Problem& P, int max_rounds, int min_rows = 4, int min_markers = 3) {
  Answer a;
  std::memset(&a.r, 0xff, sizeof(a.r));
  std::memset(&a.info, 0xff, sizeof(a.info));
  a.match.assign((size_t)P.n_cam * P.n_mk, 0xffffffffu);
  host_rig_track(P.cams.data(), P.n_cam, P.mk.data(), P.n_mk, P.beg.data(), P.det.data(), P.tol_m.data(), P.tol_a.data(),
                 P.T_pred.a, max_rounds, min_rows, min_markers, &a.r, a.match.data(), &a.info);
  return a;
}
}  // namespace

int main() {
  std::mt19937 g(20241020);
  long n_rigs = 0, n_pinned = 0, n_none = 0, rows_most = 0;
  for (int it = 0; it < 80; ++it) {
    int n_cam = 1 + (int)(g() % MPE_RIG_MAX_CAMERAS), n_mk = 4 + (int)(g() % (MPE_MAX_MARKERS - 3));
    if (it == 0) n_cam = 16, n_mk = 16;
    if (it == 1) n_cam = 1, n_mk = 4;
    if (it == 2) n_cam = 3, n_mk = 5;
    std::vector<int> seen(n_cam), stray(n_cam);
    for (int c = 0; c < n_cam; ++c) {
      seen[c] = (n_cam == 1 || c == 0) ? n_mk : (int)(g() % (n_mk + 1));
      stray[c] = (int)(g() % 6);
    }
    if (it == 0)  // 65 rows of 256 pairs: 16 + 0 + 5 + 8 + 9 * 4; camera 1 without a detection, camera 2 with 64
      for (int c = 0; c < n_cam; ++c) {
        seen[c] = c == 0 ? 16 : c == 1 ? 0 : c == 2 ? 5 : c == 3 ? 8 : c < 13 ? 4 : 0;
        stray[c] = c == 1 ? 0 : c == 2 ? 59 : stray[c];
      }
    const Problem P = make(g, n_cam, n_mk, seen, stray);
    for (int max_rounds = 1; max_rounds <= 2; ++max_rounds) {
      const Answer a = run(P, max_rounds);
      double worst = 0;
      for (int i = 0; i < 16; ++i) worst = std::fmax(worst, std::fabs(a.r.T[i] - P.T_true.a[i]));
      CHECK(a.r.status == MPE_FRAME_POSE && a.info.reason == 0 && a.r.n_corr == P.n_seen_rows && a.info.rows == P.n_seen_rows,
            "rig %d (%d x %d, %d rounds): status %d reason %d rows %d of %d", it, n_cam, n_mk, max_rounds, a.r.status,
            a.info.reason, a.r.n_corr, P.n_seen_rows);
      CHECK(worst < 1e-9, "rig %d: %.3g off", it, worst);
      CHECK(a.info.rounds == 1 && a.info.max_residual < 1e-6, "rig %d: rounds %d, residual %g", it, a.info.rounds, a.info.max_residual);
      // the rows match_out names, through rig_gn_refine from T_pred: the same bits
      std::vector<int> rc;
      std::vector<double> xyz, uv;
      for (int c = 0; c < n_cam; ++c)
        for (int m = 0; m < n_mk; ++m) {
          const uint32_t d = a.match[(size_t)c * n_mk + m];
          CHECK(d <= (uint32_t)(P.beg[c + 1] - P.beg[c]), "rig %d: match (%d, %d) = %u", it, c, m, d);
          if (d == 0 || d > (uint32_t)(P.beg[c + 1] - P.beg[c])) continue;
          CHECK((m < seen[c]) && (int)d == stray[c] + m + 1, "rig %d: (%d, %d) took detection %u", it, c, m, d);
          rc.push_back(c);
          xyz.insert(xyz.end(), &P.mk[3 * m], &P.mk[3 * m] + 3);
          uv.push_back(P.det[2 * (size_t)(P.beg[c] + d - 1)]);
          uv.push_back(P.det[2 * (size_t)(P.beg[c] + d - 1) + 1]);
        }
      mpe_result ref;
      std::memset(&ref, 0xee, sizeof(ref));
      host_rig_refine(P.cams.data(), n_cam, rc.data(), xyz.data(), uv.data(), (int)rc.size(), P.T_pred.a, &ref);
      CHECK(std::memcmp(&ref, &a.r, sizeof(ref)) == 0, "rig %d: the record is not rig_gn_refine's over the matched rows", it);
      ++n_pinned;
    }
    rows_most = P.n_seen_rows > rows_most ? P.n_seen_rows : rows_most;
    ++n_rigs;
  }
  // ---- no pose: T_pred comes back with a zero covariance
  for (int kind = 0; kind < 3; ++kind) {
    // 0: three rows (reason 1); 1: four rows on two markers over two cameras (reason 2); 2: a detection 9 px off its LED
    // and no other within reach (reason 4 with one round)
    std::vector<int> seen = kind == 0 ? std::vector<int>{2, 1} : kind == 1 ? std::vector<int>{2, 2} : std::vector<int>{5, 3};
    Problem P = make(g, 2, 5, seen, {2, 2});
    if (kind == 2) P.det[2 * (size_t)(P.beg[1] - 1)] += 9.0;
    const Answer a = run(P, 1);
    const int want = kind == 0 ? 1 : kind == 1 ? 2 : 4;
    CHECK(a.r.status == MPE_FRAME_NO_POSE && a.info.reason == want, "kind %d: status %d reason %d", kind, a.r.status, a.info.reason);
    CHECK(std::memcmp(a.r.T, P.T_pred.a, 12 * sizeof(double)) == 0 && a.r.T[15] == 1.0, "kind %d: T_pred comes back", kind);
    for (int i = 0; i < 36; ++i) CHECK(a.r.cov[i] == 0.0, "kind %d: cov[%d]", kind, i);
    CHECK(a.r.n_corr == a.info.rows && a.info.rows == (kind == 0 ? 3 : kind == 1 ? 4 : 8), "kind %d: rows %d", kind, a.info.rows);
    CHECK((kind == 2) == (a.info.max_residual > 3.0), "kind %d: residual %g", kind, a.info.max_residual);
    ++n_none;
  }
  if (g_failed) {
    std::printf("rig_track_host: %d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("rig_track_host ok: %ld rigs (up to %ld rows), %ld records bit-equal to rig_gn_refine, %ld without a pose, LDS %d bytes\n",
              n_rigs, rows_most, n_pinned, n_none, (int)sizeof(RigTrackLds));
  return 0;
}
#endif
