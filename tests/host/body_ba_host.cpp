// body_ba_host.cpp — the steps of mpe_body_calibrate (csrc/mpe_body_ba.h) compiled for the host (test scaffolding, CPU
// tier): the header as it is, behind mpe_rig_gn.h, mpe_rig_ba.h and the tail helpers of mpe_k3.hip (`struct T34` ..
// `#define K3_GROUP`, cut out at test time into k3_extract.inc), driven by the library's own row rules
// (csrc/mpe_body_ba_plan.h) and iteration (csrc/mpe_rig_ba_plan.h) over a back end that runs a launch as a loop over its
// blocks.  A phase of the header runs its 64 lanes one after the other here.  Two uses: a shared library for
// tests/test_body_ba_host.py (host_body_calibrate: mpe_body_calibrate's arguments without the handle, plus the record
// budget in doubles) against the numpy witness, and — with -DBODY_BA_HOST_MAIN — a stand-alone program that
// tools/host_sanitize.sh and the test build under -fsanitize=address,undefined: exact-pixel bodies of 4 .. 16 markers in
// front of 1 .. 16 cameras back to their true shape, in one chunk and in chunks of one view bit for bit, the row rules,
// a 16-camera view of 256 rows.  Prints "body_ba_host ok: ..." and returns 0, or says what failed and returns 1.
#include <algorithm>
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
#include "mpe_body_ba_dev.h"
#include "mpe_body_ba.h"
}  // namespace mpe
using namespace mpe;
#include "mpe_body_ba_plan.h"

namespace {
// a launch = a loop over its blocks; the kernels' LDS on the heap (every byte that is read has been written by a phase
// before — the sanitizer build would say otherwise)
struct HostSteps {
  BodyBaDev d;
  int linearise(int first, int count) {
    BodyBaLinLds* G = new BodyBaLinLds;
    for (int b = 0; b < count; ++b) body_ba_linearise(*G, d, first + b, first);
    delete G;
    return 0;
  }
  int reduce(int first, int count, bool restart) {
    BodyBaRedLds* G = new BodyBaRedLds;
    for (int i = 0; i < d.n_free; ++i)
      for (int j = i; j < d.n_free; ++j) body_ba_reduce(*G, d, i, j, first, count, restart ? 1 : 0);
    delete G;
    return 0;
  }
  int solve() {
    BodyBaSolveLds* G = new BodyBaSolveLds;
    body_ba_solve(*G, d);
    delete G;
    return 0;
  }
  int update(int first, int count) {
    for (int v = 0; v < count; ++v) body_ba_update_view(d, first + v, first);
    return 0;
  }
  int covariance() {
    BodyBaSolveLds* G = new BodyBaSolveLds;
    for (int i = 0; i < d.n_free; ++i) body_ba_covariance(*G, d, i);
    delete G;
    return 0;
  }
  int finish(int apply, double out2[2]) {
    RigBaFinLds* G = new RigBaFinLds;
    body_ba_finish(*G, d, apply);
    delete G;
    out2[0] = d.out[0];
    out2[1] = d.out[1];
    return 0;
  }
};
}  // namespace

// mpe_body_calibrate on the host: the arguments are taken as checked; cap_doubles: the record budget of a chunk
extern "C" int host_body_calibrate(const mpe_rig_camera* cameras, int n_cameras, const double* markers_xyz, int n_markers,
                                   const int* view_begin, const int* row_camera, const int* row_marker, const double* row_uv,
                                   int n_views, const double* T_view_init, int scale, int max_iterations,
                                   double step_tolerance, long long cap_doubles, double* markers_out, double* T_view_out,
                                   double* cov_out, int* view_used, mpe_body_calibration_report* report) {
  BodyBaPlan P;
  body_ba_plan(n_markers, view_begin, row_camera, row_marker, row_uv, n_views, MPE_BODY_BA_HEAD, MPE_BODY_BA_SLOT, P);
  const int held = body_ba_scale_held(P, scale);
  body_ba_give_back(P, held, markers_xyz, n_views, T_view_init, markers_out, T_view_out, cov_out, view_used, report);
  if (P.views_used == 0 || P.n_free < 3) return 0;
  const int nv = P.views_used, nf = P.n_free;
  std::vector<mpe_rig_camera> cams(cameras, cameras + n_cameras);
  std::vector<double> mk(markers_xyz, markers_xyz + 3 * (size_t)n_markers);
  std::vector<double> T((size_t)nv * 16), sse((size_t)nv), step((size_t)nv), Sacc((size_t)(nf * (nf + 1) / 2) * 18),
      racc((size_t)nf * 6), Lf((size_t)(3 * nf) * (3 * nf + 1) / 2), delta((size_t)3 * nf), gauge(MPE_BODY_BA_GAUGE),
      cov((size_t)nf * 9, 0.0);
  for (int v = 0; v < nv; ++v) std::memcpy(&T[(size_t)v * 16], T_view_init + 16 * (size_t)P.view_of[(size_t)v], 16 * sizeof(double));
  const std::vector<std::pair<int, int>> chunks = rig_ba_chunks(P, cap_doubles);
  long long rec_doubles = 0;
  for (const auto& c : chunks)
    rec_doubles = std::max(rec_doubles, P.view_cum[(size_t)(c.first + c.second)] - P.view_cum[(size_t)c.first]);
  std::vector<double> rec((size_t)rec_doubles);  // (exactly what the plan says a chunk needs: a step that writes past it is caught)
  double out2[2] = {0, 0};
  HostSteps B;
  B.d.cams = cams.data();
  B.d.free_marker = P.free_marker;
  B.d.n_cam = n_cameras, B.d.n_free = nf, B.d.n_views = nv;
  B.d.scale_held = held;
  B.d.view_begin = P.view_begin.data();
  B.d.view_mask = P.view_mask.data();
  B.d.view_cum = P.view_cum.data();
  B.d.row_cam = P.row_cam.data();
  B.d.row_free = P.row_free.data();
  B.d.row_uv = P.row_uv.data();
  B.d.markers = mk.data();
  B.d.T_view = T.data();
  B.d.rec = rec.data();
  B.d.sse = sse.data();
  B.d.step = step.data();
  B.d.Sacc = Sacc.data();
  B.d.racc = racc.data();
  B.d.Lf = Lf.data();
  B.d.delta = delta.data();
  B.d.gauge = gauge.data();
  B.d.cov = cov.data();
  B.d.out = out2;
  RigBaOutcome o;
  rig_ba_iterate(B, chunks, max_iterations, step_tolerance, o);
  return body_ba_hand_out(P, o, mk.data(), T.data(), cov.data(), markers_out, T_view_out, cov_out, report);
}

#ifdef BODY_BA_HOST_MAIN
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

// n_mk markers in front of n_cam cameras in n_views views, every (camera, marker) row there with probability 1 -
// p_missing (exact pixels); start markers `off` metres off per component
struct Problem {
  std::vector<mpe_rig_camera> cams;
  std::vector<M4> T_start;
  std::vector<int> begin, rc, rm;
  std::vector<double> truth, start, uv;
};
Problem make(std::mt19937& g, int n_cam, int n_views, int n_mk, double p_missing, double off) {
  std::uniform_real_distribution<double> ud(0.0, 1.0);
  Problem P;
  P.truth.resize(3 * (size_t)n_mk);
  for (double& v : P.truth) v = 0.3 * (2 * ud(g) - 1);
  P.start = P.truth;
  for (double& v : P.start) v += off * (2 * ud(g) - 1);
  std::vector<M4> E;
  P.cams.resize(n_cam);
  for (int c = 0; c < n_cam; ++c) {
    std::memset(&P.cams[c], 0, sizeof(P.cams[c]));
    P.cams[c].K[0] = 420 + 20 * ud(g), P.cams[c].K[4] = 425 + 20 * ud(g), P.cams[c].K[2] = 370, P.cams[c].K[5] = 235, P.cams[c].K[8] = 1;
    M4 Ec = rigid(g, n_cam == 1 ? 0.0 : 0.5, n_cam == 1 ? 0.0 : 0.3);
    E.push_back(Ec);
    std::memcpy(P.cams[c].T_cam_rig, Ec.a, sizeof(Ec.a));
  }
  P.begin.push_back(0);
  for (int f = 0; f < n_views; ++f) {
    M4 T = rigid(g, 1.2, 0.2);
    T.a[11] += 1.5;
    for (int c = 0; c < n_cam; ++c)
      for (int m = 0; m < n_mk; ++m) {
        if (ud(g) < p_missing) continue;
        double X[3], q[3];
        apply(T, &P.truth[3 * (size_t)m], X);
        apply(E[c], X, q);
        P.rc.push_back(c);
        P.rm.push_back(m);
        P.uv.push_back(P.cams[c].K[0] * q[0] / q[2] + P.cams[c].K[2]);
        P.uv.push_back(P.cams[c].K[4] * q[1] / q[2] + P.cams[c].K[5]);
      }
    P.begin.push_back((int)P.rc.size());
    P.T_start.push_back(mul(rigid(g, 0.05, 0.01), T));
  }
  return P;
}

struct Answer {
  int rc;
  std::vector<double> mk, T, cov;
  std::vector<int> used;
  mpe_body_calibration_report rep;
};
Answer run(const Problem& P, int scale, long long cap) {
  const int n_cam = (int)P.cams.size(), n_views = (int)P.T_start.size(), n_mk = (int)P.start.size() / 3;
  Answer A;
  A.mk.assign((size_t)n_mk * 3, -7.0);
  A.T.assign((size_t)n_views * 16, -7.0);
  A.cov.assign((size_t)n_mk * 9, -7.0);
  A.used.assign((size_t)n_views, -7);
  A.rc = host_body_calibrate(P.cams.data(), n_cam, P.start.data(), n_mk, P.begin.data(), P.rc.data(), P.rm.data(), P.uv.data(),
                             n_views, P.T_start[0].a, scale, 50, 1e-10, cap, A.mk.data(), A.T.data(), A.cov.data(),
                             A.used.data(), &A.rep);
  return A;
}

// the largest difference of a pairwise distance between two shapes, relative to `scale_free` (divide by the mean distance)
double distances_off(const std::vector<double>& a, const std::vector<double>& b, const int* state, bool scale_free) {
  const int n = (int)a.size() / 3;
  double sa = 0, sb = 0, worst = 0;
  auto dist = [](const std::vector<double>& p, int i, int j) {
    return std::sqrt((p[3 * i] - p[3 * j]) * (p[3 * i] - p[3 * j]) + (p[3 * i + 1] - p[3 * j + 1]) * (p[3 * i + 1] - p[3 * j + 1]) +
                     (p[3 * i + 2] - p[3 * j + 2]) * (p[3 * i + 2] - p[3 * j + 2]));
  };
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if (state[i] == 1 && state[j] == 1) sa += dist(a, i, j), sb += dist(b, i, j);
  const double k = scale_free ? sb / sa : 1.0;
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if (state[i] == 1 && state[j] == 1) worst = std::fmax(worst, std::fabs(k * dist(a, i, j) - dist(b, i, j)));
  return worst;
}
}  // namespace

int main() {
  std::mt19937 g(20240913);
  long n_bodies = 0, n_chunked = 0, rows_most = 0;
  static_assert(sizeof(M4) == 16 * sizeof(double), "the start poses are handed over as one array");
  for (int it = 0; it < 40; ++it) {
    int n_cam = 1 + (int)(g() % 6), n_views = 6 + (int)(g() % 30), n_mk = 4 + (int)(g() % 5);
    double p_missing = 0.15;
    if (it == 0) n_cam = 16, n_views = 3, n_mk = 16, p_missing = 0;  // 256 rows a view, a 48 x 48 reduced system
    if (it == 1) n_cam = 1, n_views = 6, n_mk = 4, p_missing = 0;
    if (it == 2) n_cam = 3, n_views = 70, n_mk = 5;                 // more views than a wave has lanes
    const Problem P = make(g, n_cam, n_views, n_mk, p_missing, 0.004);
    const Answer A = run(P, -1, 1LL << 40);
    if (A.rep.views_used == 0) continue;
    CHECK(A.rc == 1 && A.rep.status == MPE_FRAME_POSE, "body %d: rc %d status %d", it, A.rc, A.rep.status);
    CHECK(A.rep.iterations >= 2 && A.rep.iterations <= 12, "body %d: %d iterations", it, A.rep.iterations);
    CHECK(A.rep.rms_after <= 1e-9 && A.rep.rms_after <= A.rep.rms_before, "body %d: rms %g -> %g", it, A.rep.rms_before,
          A.rep.rms_after);
    CHECK(A.rep.scale_held == (n_cam == 1 ? 1 : A.rep.scale_held), "body %d: one camera holds the scale", it);
    const double worst = distances_off(A.mk, P.truth, A.rep.marker_state, A.rep.scale_held != 0);
    CHECK(worst < 1e-9, "body %d (%d cameras, %d views, %d markers): shape %.3g off", it, n_cam, n_views, n_mk, worst);
    double shift[3] = {0, 0, 0};
    for (int m = 0; m < n_mk; ++m) {
      if (A.rep.marker_state[m] == 2) {
        CHECK(std::memcmp(&A.mk[3 * (size_t)m], &P.start[3 * (size_t)m], 3 * sizeof(double)) == 0, "body %d: held marker %d moved", it, m);
        for (int i = 0; i < 9; ++i) CHECK(A.cov[9 * (size_t)m + i] == 0, "body %d: cov of held marker %d", it, m);
        continue;
      }
      for (int k = 0; k < 3; ++k) shift[k] += A.mk[3 * (size_t)m + k] - P.start[3 * (size_t)m + k];
      for (int i = 0; i < 3; ++i) CHECK(A.cov[9 * (size_t)m + 4 * i] > 0, "body %d marker %d: variance %d", it, m, i);
    }
    for (int k = 0; k < 3; ++k) CHECK(std::fabs(shift[k]) <= 1e-12, "body %d: the centroid moved by %.3g", it, shift[k]);
    for (int f = 0; f < n_views; ++f) {
      rows_most = std::max<long>(rows_most, P.begin[f + 1] - P.begin[f]);
      if (!A.used[f]) CHECK(std::memcmp(&A.T[(size_t)f * 16], P.T_start[f].a, 16 * sizeof(double)) == 0, "body %d: unused view %d moved", it, f);
    }
    ++n_bodies;
    // the same problem with a chunk per view: the same bits
    if (it % 4 == 0 || it < 3) {
      const Answer B = run(P, -1, 1);
      CHECK(B.rc == A.rc && B.rep.iterations == A.rep.iterations, "body %d chunked: rc / iterations", it);
      CHECK(B.mk == A.mk && B.T == A.T && B.cov == A.cov && B.used == A.used, "body %d chunked: outputs differ", it);
      CHECK(B.rep.rms_before == A.rep.rms_before && B.rep.rms_after == A.rep.rms_after && B.rep.last_step == A.rep.last_step,
            "body %d chunked: report differs", it);
      ++n_chunked;
    }
  }
  // ---- the rules: a view of 3 rows, a marker with one row, fewer than 3 free markers
  {
    Problem P = make(g, 2, 12, 6, 0.0, 0.004);
    Problem Q = P;
    Q.begin.assign(1, 0), Q.rc.clear(), Q.rm.clear(), Q.uv.clear();
    for (int f = 0; f < 12; ++f) {
      int kept = 0;
      for (int j = P.begin[f]; j < P.begin[f + 1]; ++j) {
        if (P.rm[j] == 5 && !(f == 2 && P.rc[j] == 0)) continue;  // marker 5: one row in all
        if (f == 7 && kept >= 3) continue;                         // view 7: three rows
        Q.rc.push_back(P.rc[j]), Q.rm.push_back(P.rm[j]);
        Q.uv.push_back(P.uv[2 * (size_t)j]), Q.uv.push_back(P.uv[2 * (size_t)j + 1]);
        ++kept;
      }
      Q.begin.push_back((int)Q.rc.size());
    }
    const Answer A = run(Q, -1, 1LL << 40);
    CHECK(A.rc == 1 && A.rep.markers_free == 5 && A.rep.marker_state[5] == 2 && A.rep.marker_rows[5] == 0, "rules: marker 5 state %d rows %d",
          A.rep.marker_state[5], A.rep.marker_rows[5]);
    CHECK(A.rep.views_used == 11 && A.rep.rows_used == 110 && A.rep.scale_held == 0, "rules: %d views, %d rows", A.rep.views_used, A.rep.rows_used);
    for (int f = 0; f < 12; ++f) CHECK(A.used[f] == (f != 7 ? 1 : 0), "rules: view %d used %d", f, A.used[f]);
    CHECK(std::memcmp(&A.mk[15], &Q.start[15], 3 * sizeof(double)) == 0, "rules: the held marker moved");
    CHECK(distances_off(A.mk, Q.truth, A.rep.marker_state, false) < 1e-9, "rules: shape off");
    // two markers only: nothing is calibrated, everything comes back as given
    Problem R = P;
    R.begin.assign(1, 0), R.rc.clear(), R.rm.clear(), R.uv.clear();
    for (int f = 0; f < 12; ++f) {
      for (int j = P.begin[f]; j < P.begin[f + 1]; ++j) {
        if (P.rm[j] > 1) continue;
        R.rc.push_back(P.rc[j]), R.rm.push_back(P.rm[j]);
        R.uv.push_back(P.uv[2 * (size_t)j]), R.uv.push_back(P.uv[2 * (size_t)j + 1]);
      }
      R.begin.push_back((int)R.rc.size());
    }
    const Answer Z = run(R, -1, 1LL << 40);
    CHECK(Z.rc == 0 && Z.rep.status == MPE_FRAME_NO_POSE && Z.rep.markers_free == 0 && Z.rep.views_used == 0, "rules: two markers");
    CHECK(Z.mk == R.start, "rules: two markers: the markers come back as given");
    for (int f = 0; f < 12; ++f) CHECK(std::memcmp(&Z.T[(size_t)f * 16], R.T_start[f].a, 16 * sizeof(double)) == 0, "rules: view %d moved", f);
  }
  if (g_failed) {
    std::printf("body_ba_host: %d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("body_ba_host ok: %ld bodies back to their shape (up to %ld rows a view), %ld of them again in chunks of one view bit for bit, the row rules\n",
              n_bodies, rows_most, n_chunked);
  return 0;
}
#endif
