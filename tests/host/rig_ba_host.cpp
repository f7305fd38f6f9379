// rig_ba_host.cpp — the steps of mpe_rig_calibrate (csrc/mpe_rig_ba.h) compiled for the host (test scaffolding, CPU tier):
// the header as it is, behind mpe_rig_gn.h and the tail helpers of mpe_k3.hip (`struct T34` .. `#define K3_GROUP`, cut
// out at test time into k3_extract.inc), driven by the library's own row rules and iteration (csrc/mpe_rig_ba_plan.h)
// over a back end that runs a launch as a loop over its blocks.  A phase of the header runs its 64 lanes one after the
// other here.  Two uses: a shared library for tests/test_rig_ba_host.py (host_rig_calibrate: mpe_rig_calibrate's
// arguments without the handle, plus the record budget in doubles) against the numpy witness, and — with
// -DRIG_BA_HOST_MAIN — a stand-alone program that tools/host_sanitize.sh and the test build under
// -fsanitize=address,undefined: exact-pixel rigs of 2 .. 16 cameras back to their true extrinsics, in one chunk and in
// chunks of one view bit for bit, the row rules, a 16-camera view of 256 rows.  Prints "rig_ba_host ok: ..." and returns
// 0, or says what failed and returns 1.
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
#include "mpe_rig_ba_dev.h"
#include "mpe_rig_ba.h"
}  // namespace mpe
using namespace mpe;
#include "mpe_rig_ba_plan.h"

namespace {
// a launch = a loop over its blocks; the kernels' LDS on the heap (every byte that is read has been written by a phase
// before — the sanitizer build would say otherwise)
struct HostSteps {
  RigBaDev d;
  int linearise(int first, int count) {
    RigBaLinLds* G = new RigBaLinLds;
    for (int b = 0; b < count; ++b) rig_ba_linearise(*G, d, first + b, first);
    delete G;
    return 0;
  }
  int reduce(int first, int count, bool restart) {
    RigBaRedLds* G = new RigBaRedLds;
    for (int i = 0; i < d.n_free; ++i)
      for (int j = i; j < d.n_free; ++j) rig_ba_reduce(*G, d, i, j, first, count, restart ? 1 : 0);
    delete G;
    return 0;
  }
  int solve() {
    RigBaSolveLds* G = new RigBaSolveLds;
    rig_ba_solve(*G, d);
    delete G;
    return 0;
  }
  int update(int first, int count) {
    for (int v = 0; v < count; ++v) rig_ba_update_view(d, first + v, first);
    return 0;
  }
  int covariance() {
    RigBaSolveLds* G = new RigBaSolveLds;
    for (int i = 0; i < d.n_free; ++i) rig_ba_covariance(*G, d, i);
    delete G;
    return 0;
  }
  int finish(int apply, double out2[2]) {
    RigBaFinLds* G = new RigBaFinLds;
    rig_ba_finish(*G, d, apply);
    delete G;
    out2[0] = d.out[0];
    out2[1] = d.out[1];
    return 0;
  }
};
}  // namespace

// mpe_rig_calibrate on the host: the arguments are taken as checked; cap_doubles: the record budget of a chunk
extern "C" int host_rig_calibrate(const mpe_rig_camera* cameras, int n_cameras, const int* view_begin, const int* row_camera,
                                  const double* row_marker_xyz, const double* row_uv, int n_views, const double* T_view_init,
                                  int reference_camera, int max_iterations, double step_tolerance, long long cap_doubles,
                                  double* T_cam_rig_out, double* T_view_out, double* cov_out, int* view_used,
                                  mpe_rig_calibration_report* report) {
  RigBaPlan P;
  rig_ba_plan(n_cameras, reference_camera, view_begin, row_camera, row_marker_xyz, row_uv, n_views, MPE_RIG_BA_HEAD,
              MPE_RIG_BA_SLOT, P);
  rig_ba_give_back(P, cameras, n_views, T_view_init, T_cam_rig_out, T_view_out, cov_out, view_used, report);
  if (P.views_used == 0 || P.n_free == 0) return 0;
  const int nv = P.views_used, nf = P.n_free;
  std::vector<mpe_rig_camera> cams(cameras, cameras + n_cameras);
  std::vector<double> T((size_t)nv * 16), sse((size_t)nv), step((size_t)nv), Sacc((size_t)(nf * (nf + 1) / 2) * 72),
      racc((size_t)nf * 12), Lf((size_t)(6 * nf) * (6 * nf + 1) / 2), eta((size_t)6 * nf), cov((size_t)nf * 36, 0.0);
  for (int v = 0; v < nv; ++v) std::memcpy(&T[(size_t)v * 16], T_view_init + 16 * (size_t)P.view_of[(size_t)v], 16 * sizeof(double));
  const std::vector<std::pair<int, int>> chunks = rig_ba_chunks(P, cap_doubles);
  long long rec_doubles = 0;
  for (const auto& c : chunks)
    rec_doubles = std::max(rec_doubles, P.view_cum[(size_t)(c.first + c.second)] - P.view_cum[(size_t)c.first]);
  std::vector<double> rec((size_t)rec_doubles);  // (exactly what the plan says a chunk needs: a step that writes past it is caught)
  double out2[2] = {0, 0};
  HostSteps B;
  B.d.cams = cams.data();
  B.d.cam_free = P.cam_free;
  B.d.n_cam = n_cameras, B.d.n_free = nf, B.d.n_views = nv;
  B.d.view_begin = P.view_begin.data();
  B.d.view_mask = P.view_mask.data();
  B.d.view_cum = P.view_cum.data();
  B.d.row_cam = P.row_cam.data();
  B.d.row_xyz = P.row_xyz.data();
  B.d.row_uv = P.row_uv.data();
  B.d.T_view = T.data();
  B.d.rec = rec.data();
  B.d.sse = sse.data();
  B.d.step = step.data();
  B.d.Sacc = Sacc.data();
  B.d.racc = racc.data();
  B.d.Lf = Lf.data();
  B.d.eta = eta.data();
  B.d.cov = cov.data();
  B.d.out = out2;
  RigBaOutcome o;
  rig_ba_iterate(B, chunks, max_iterations, step_tolerance, o);
  return rig_ba_hand_out(P, o, cams.data(), T.data(), cov.data(), T_cam_rig_out, T_view_out, cov_out, report);
}

#ifdef RIG_BA_HOST_MAIN
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

// a rig of n_cam cameras, n_views views, every camera sees `per` markers in every view it is in (exact pixels)
struct Problem {
  std::vector<mpe_rig_camera> start;
  std::vector<M4> E_true, T_start;
  std::vector<int> begin, rc;
  std::vector<double> xyz, uv;
};
Problem make(std::mt19937& g, int n_cam, int n_views, int per, double p_missing, int ref) {
  std::uniform_real_distribution<double> ud(0.0, 1.0);
  Problem P;
  std::vector<double> mk(3 * MPE_MAX_MARKERS);
  for (double& v : mk) v = 0.3 * (2 * ud(g) - 1);
  std::vector<mpe_rig_camera> cams(n_cam);
  for (int c = 0; c < n_cam; ++c) {
    std::memset(&cams[c], 0, sizeof(cams[c]));
    cams[c].K[0] = 420 + 20 * ud(g), cams[c].K[4] = 425 + 20 * ud(g), cams[c].K[2] = 370, cams[c].K[5] = 235, cams[c].K[8] = 1;
    P.E_true.push_back(rigid(g, 0.5, 0.3));
    const M4 Es = c == ref ? P.E_true[c] : mul(rigid(g, 0.03, 0.005), P.E_true[c]);
    std::memcpy(cams[c].T_cam_rig, Es.a, sizeof(Es.a));
  }
  P.start = cams;
  P.begin.push_back(0);
  for (int f = 0; f < n_views; ++f) {
    M4 T = rigid(g, 0.6, 0.2);
    T.a[11] += 1.5;
    for (int c = 0; c < n_cam; ++c) {
      if (ud(g) < p_missing) continue;
      for (int j = 0; j < per; ++j) {
        double X[3], q[3];
        apply(T, &mk[3 * j], X);
        apply(P.E_true[c], X, q);
        P.rc.push_back(c);
        P.xyz.insert(P.xyz.end(), &mk[3 * j], &mk[3 * j] + 3);
        P.uv.push_back(cams[c].K[0] * q[0] / q[2] + cams[c].K[2]);
        P.uv.push_back(cams[c].K[4] * q[1] / q[2] + cams[c].K[5]);
      }
    }
    P.begin.push_back((int)P.rc.size());
    P.T_start.push_back(mul(rigid(g, 0.05, 0.01), T));
  }
  return P;
}

struct Answer {
  int rc;
  std::vector<double> E, T, cov;
  std::vector<int> used;
  mpe_rig_calibration_report rep;
};
Answer run(const Problem& P, int ref, long long cap) {
  const int n_cam = (int)P.start.size(), n_views = (int)P.T_start.size();
  Answer A;
  A.E.assign((size_t)n_cam * 16, -7.0);
  A.T.assign((size_t)n_views * 16, -7.0);
  A.cov.assign((size_t)n_cam * 36, -7.0);
  A.used.assign((size_t)n_views, -7);
  A.rc = host_rig_calibrate(P.start.data(), n_cam, P.begin.data(), P.rc.data(), P.xyz.data(), P.uv.data(), n_views,
                            P.T_start[0].a, ref, 50, 1e-10, cap, A.E.data(), A.T.data(), A.cov.data(), A.used.data(), &A.rep);
  return A;
}
}  // namespace

int main() {
  std::mt19937 g(20240911);
  long n_rigs = 0, n_chunked = 0, rows_most = 0;
  static_assert(sizeof(M4) == 16 * sizeof(double), "the start poses are handed over as one array");
  for (int it = 0; it < 40; ++it) {
    int n_cam = 2 + (int)(g() % 7), n_views = 3 + (int)(g() % 30), per = 4 + (int)(g() % 2), ref = 0;
    double p_missing = 0.25;
    if (it == 0) n_cam = 16, n_views = 3, per = 16, p_missing = 0;  // 256 rows a view, a 90 x 90 reduced system
    if (it == 1) n_cam = 2, n_views = 2, per = 4, p_missing = 0;
    if (it == 2) n_cam = 3, n_views = 70, per = 4;                  // more views than a wave has lanes
    if (it >= 30) ref = (int)(g() % n_cam);
    const Problem P = make(g, n_cam, n_views, per, p_missing, ref);
    const Answer A = run(P, ref, 1LL << 40);
    CHECK(A.rep.camera_state[ref] == 0, "rig %d: the reference camera's state", it);
    if (A.rep.views_used == 0) continue;  // (nothing links: as the rules say)
    CHECK(A.rc == 1 && A.rep.status == MPE_FRAME_POSE, "rig %d: rc %d status %d", it, A.rc, A.rep.status);
    CHECK(A.rep.iterations >= 2 && A.rep.iterations <= 10, "rig %d: %d iterations", it, A.rep.iterations);
    CHECK(A.rep.rms_after <= 1e-9 && A.rep.rms_after <= A.rep.rms_before, "rig %d: rms %g -> %g", it, A.rep.rms_before,
          A.rep.rms_after);
    double worst = 0;
    for (int c = 0; c < n_cam; ++c) {
      if (A.rep.camera_state[c] == 2) {
        CHECK(std::memcmp(&A.E[(size_t)c * 16], P.start[c].T_cam_rig, 16 * sizeof(double)) == 0, "rig %d: held camera %d moved", it, c);
        continue;
      }
      for (int i = 0; i < 16; ++i) worst = std::fmax(worst, std::fabs(A.E[(size_t)c * 16 + i] - P.E_true[c].a[i]));
      if (A.rep.camera_state[c] == 1)
        for (int i = 0; i < 6; ++i) CHECK(A.cov[(size_t)c * 36 + 7 * i] > 0, "rig %d camera %d: variance %d", it, c, i);
    }
    CHECK(worst < 1e-9, "rig %d (%d cameras, %d views): extrinsics %.3g off", it, n_cam, n_views, worst);
    for (int f = 0; f < n_views; ++f) {
      rows_most = std::max<long>(rows_most, P.begin[f + 1] - P.begin[f]);
      if (!A.used[f]) CHECK(std::memcmp(&A.T[(size_t)f * 16], P.T_start[f].a, 16 * sizeof(double)) == 0, "rig %d: unused view %d moved", it, f);
    }
    ++n_rigs;
    // the same problem with a chunk per view: the same bits
    if (it % 4 == 0 || it < 3) {
      const Answer B = run(P, ref, 1);
      CHECK(B.rc == A.rc && B.rep.iterations == A.rep.iterations, "rig %d chunked: rc / iterations", it);
      CHECK(B.E == A.E && B.T == A.T && B.cov == A.cov && B.used == A.used, "rig %d chunked: outputs differ", it);
      CHECK(B.rep.rms_before == A.rep.rms_before && B.rep.rms_after == A.rep.rms_after && B.rep.last_step == A.rep.last_step,
            "rig %d chunked: report differs", it);
      ++n_chunked;
    }
  }
  // ---- the rules: a view of one camera, a view of 2 rows, a camera without rows, a camera linked to nobody
  {
    Problem P = make(g, 4, 12, 4, 0.0, 0);
    // camera 3 only ever together with nobody: move its rows into views of their own
    Problem Q;
    Q.start = P.start, Q.E_true = P.E_true;
    Q.begin.push_back(0);
    for (int f = 0; f < 12; ++f) {
      for (int pass = 0; pass < 2; ++pass) {
        for (int j = P.begin[f]; j < P.begin[f + 1]; ++j) {
          const bool lone = P.rc[j] == 3;
          if (lone != (pass == 1) || P.rc[j] == 2) continue;  // (camera 2 brings no row at all)
          if (f == 5 && pass == 0 && (P.rc[j] != 0 || j - P.begin[f] >= 2)) continue;  // view 5: two rows of camera 0
          Q.rc.push_back(P.rc[j]);
          Q.xyz.insert(Q.xyz.end(), &P.xyz[3 * (size_t)j], &P.xyz[3 * (size_t)j] + 3);
          Q.uv.insert(Q.uv.end(), &P.uv[2 * (size_t)j], &P.uv[2 * (size_t)j] + 2);
        }
        Q.begin.push_back((int)Q.rc.size());
        Q.T_start.push_back(P.T_start[f]);
      }
    }
    const Answer A = run(Q, 0, 1LL << 40);
    CHECK(A.rc == 1 && A.rep.camera_state[0] == 0 && A.rep.camera_state[1] == 1 && A.rep.camera_state[2] == 2 &&
              A.rep.camera_state[3] == 2, "rules: states %d %d %d %d", A.rep.camera_state[0], A.rep.camera_state[1],
          A.rep.camera_state[2], A.rep.camera_state[3]);
    CHECK(A.rep.views_used == 11 && A.rep.rows_used == 88 && A.rep.camera_rows[2] == 0 && A.rep.camera_rows[3] == 0,
          "rules: %d views, %d rows", A.rep.views_used, A.rep.rows_used);
    for (int f = 0; f < 24; ++f) CHECK(A.used[f] == ((f % 2 == 0 && f != 10) ? 1 : 0), "rules: view %d used %d", f, A.used[f]);
    for (int c = 2; c < 4; ++c)
      CHECK(std::memcmp(&A.E[(size_t)c * 16], Q.start[c].T_cam_rig, 16 * sizeof(double)) == 0, "rules: held camera %d moved", c);
    double worst = 0;
    for (int i = 0; i < 16; ++i) worst = std::fmax(worst, std::fabs(A.E[16 + i] - Q.E_true[1].a[i]));
    CHECK(worst < 1e-9, "rules: camera 1 %.3g off", worst);
    for (int i = 0; i < 36; ++i) CHECK(A.cov[i] == 0 && A.cov[72 + i] == 0 && A.cov[108 + i] == 0, "rules: cov[%d] of a fixed camera", i);
  }
  if (g_failed) {
    std::printf("rig_ba_host: %d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("rig_ba_host ok: %ld rigs back to their extrinsics (up to %ld rows a view), %ld of them again in chunks of one view bit for bit, the row rules\n",
              n_rigs, rows_most, n_chunked);
  return 0;
}
#endif
