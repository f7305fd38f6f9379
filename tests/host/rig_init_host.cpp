// rig_init_host.cpp — the logic of the rig initialiser (csrc/mpe_rig_init.h) compiled for the host (test scaffolding, CPU
// tier): the header as it is, behind mpe_p3p.h, the index helpers of mpe_k2_head.h (`unrank_combo3` .. `pick_root`, cut out
// at test time into k2_head_extract.inc), the tail helpers of mpe_k3.hip (k3_extract.inc, as tests/host/rig_track_host.cpp
// has them), mpe_rig_gn.h and mpe_rig_track.h.  The device spreads the items over blocks of 128 lanes; here ONE lane takes
// them one after the other, `chunk` items at a time with a key per chunk, the keys reduced afterwards as the device's
// second launch does.  Two uses: a shared library for tests/test_rig_init_host.py (host_rig_init against the numpy
// witness) and tools/rig_init_probe.py (the single-core time), and — with -DRIG_INIT_HOST_MAIN — a stand-alone program that
// the test builds plain and under -fsanitize=address,undefined: the unranking against nested loops, rigs of 2 .. 4 cameras
// that see [3, 3, 2]-like shares of 5 LEDs (exact pixels among stray detections) back to their true pose, the result
// independent of the chunk size, and the problems without a pose.  Prints "rig_init_host ok: ..." and returns 0, or says
// what failed and returns 1.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include <hip/hip_runtime.h>  // (tests/host/stub: the one-lane meaning of the HIP spellings)

#include "../../include/mpe.h"
#include "mpe_p3p.h"
namespace mpe {
#include "k2_head_extract.inc"
#include "k3_extract.inc"
#include "mpe_rig_gn.h"
#include "mpe_rig_track.h"
#include "mpe_rig_init.h"
}  // namespace mpe
using namespace mpe;

// chunk <= 0: MPE_RIG_INIT_CHUNK
extern "C" void host_rig_init_chunked(const mpe_rig_camera* cams, int n_cam, const double* markers, int n_mk,
                                      const int* det_begin, const double* det_xy, const double* tol_vote,
                                      const double* tol_accept, int max_rounds, int min_rows, int min_markers, int min_margin,
                                      int chunk, mpe_result* out, uint32_t* match, mpe_rig_init_info* info) {
  if (chunk <= 0) chunk = MPE_RIG_INIT_CHUNK;
  RigInitLds* S = new RigInitLds;  // (the kernel's LDS; every byte that is read has been written before)
  unsigned char W[MPE_RIG_MAX_ROWS];
  rig_init_stage(*S, 0, 1, cams, n_cam, markers, n_mk, det_begin, det_xy, tol_vote, nullptr);
  const int n_items = S->off[n_cam];
  std::vector<RigInitKey> keys;
  int unused = 0;
  for (int first = 0; first < n_items; first += chunk) {
    RigInitKey key = rig_init_no_key();
    for (int item = first; item < n_items && item < first + chunk; ++item) rig_init_item(*S, 0, n_cam, n_mk, item, 0, key, unused);
    keys.push_back(key);
  }
  RigInitKey win = rig_init_no_key();
  for (const RigInitKey& k : keys)
    if (rig_init_better(k, win)) win = k;
  rig_init_winner(*S, 0, n_cam, n_mk, win, W, info);
  int runner = 0;
  if (win.h >= 0) {
    rig_init_stage(*S, 0, 1, cams, n_cam, markers, n_mk, det_begin, det_xy, tol_vote, W);
    RigInitKey none = rig_init_no_key();
    for (int item = 0; item < n_items; ++item) rig_init_item(*S, 0, n_cam, n_mk, item, 1, none, runner);
  }
  delete S;
  RigTrackLds* T = new RigTrackLds;
  rig_init_finish(*T, cams, n_cam, markers, n_mk, det_begin, det_xy, tol_vote, tol_accept, W, runner, max_rounds, min_rows,
                  min_markers, min_margin, out, match, info);
  delete T;
}

extern "C" void host_rig_init(const mpe_rig_camera* cams, int n_cam, const double* markers, int n_mk, const int* det_begin,
                              const double* det_xy, const double* tol_vote, const double* tol_accept, int max_rounds,
                              int min_rows, int min_markers, int min_margin, mpe_result* out, uint32_t* match,
                              mpe_rig_init_info* info) {
  host_rig_init_chunked(cams, n_cam, markers, n_mk, det_begin, det_xy, tol_vote, tol_accept, max_rounds, min_rows, min_markers,
                        min_margin, 0, out, match, info);
}

extern "C" int host_rig_init_lds_bytes() { return (int)sizeof(RigInitLds); }

// item -> out7 = (camera, detection triple, marker triple) of a problem with these list lengths
extern "C" void host_rig_init_decode(const int* n_det, int n_cam, int n_mk, int item, int* out7) {
  RigInitLds* S = new RigInitLds;
  S->beg[0] = S->off[0] = 0;
  for (int c = 0; c < n_cam; ++c) {
    S->beg[c + 1] = S->beg[c] + n_det[c];
    S->off[c + 1] = S->off[c] + rig_init_camera_items(n_det[c], n_mk);
  }
  RigInitItem it;
  rig_init_decode(*S, n_mk, item, it);
  const int v[7] = {it.cam, it.d[0], it.d[1], it.d[2], it.m[0], it.m[1], it.m[2]};
  std::memcpy(out7, v, sizeof(v));
  delete S;
}

#ifdef RIG_INIT_HOST_MAIN
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
void apply(const M4& T, const double* p, double* q) {
  for (int i = 0; i < 3; ++i) q[i] = T.a[4 * i] * p[0] + T.a[4 * i + 1] * p[1] + T.a[4 * i + 2] * p[2] + T.a[4 * i + 3];
}

struct Problem {
  std::vector<mpe_rig_camera> cams;
  std::vector<double> mk, det, tol;
  std::vector<int> beg;
  M4 T_true;
  int n_cam, n_mk, n_seen_rows;
};
// camera c sees the markers first[c] .. first[c] + seen[c] - 1 (mod n_mk; exact pixels) among stray[c] stray detections
Problem make(std::mt19937& g, int n_cam, int n_mk, const std::vector<int>& first, const std::vector<int>& seen,
             const std::vector<int>& stray) {
  std::uniform_real_distribution<double> ud(0.0, 1.0);
  Problem P;
  P.n_cam = n_cam, P.n_mk = n_mk, P.n_seen_rows = 0;
  P.cams.resize(n_cam);
  P.mk.resize(3 * n_mk);
  for (double& v : P.mk) v = 0.5 * (2 * ud(g) - 1);
  P.T_true = rigid(g, 0.6, 0.2);
  P.T_true.a[11] += 1.8;
  P.beg.assign(1, 0);
  for (int c = 0; c < n_cam; ++c) {
    mpe_rig_camera& cam = P.cams[c];
    std::memset(&cam, 0, sizeof(cam));
    cam.K[0] = 420 + 20 * ud(g), cam.K[4] = 425 + 20 * ud(g), cam.K[2] = 370, cam.K[5] = 235, cam.K[8] = 1;
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
    for (int k = 0; k < stray[c];) {
      const double x = 2000 * ud(g) - 600, y = 1500 * ud(g) - 500;
      bool far = true;
      for (int m = 0; m < n_mk; ++m) far = far && std::hypot(x - led[2 * m], y - led[2 * m + 1]) > 40.0;
      if (!far) continue;
      P.det.push_back(x), P.det.push_back(y);
      ++k;
    }
    for (int k = 0; k < seen[c]; ++k) {
      const int m = (first[c] + k) % n_mk;
      P.det.push_back(led[2 * m]), P.det.push_back(led[2 * m + 1]);
    }
    P.n_seen_rows += seen[c];
    P.beg.push_back((int)P.det.size() / 2);
  }
  P.tol.assign(n_cam, 3.0);
  return P;
}
struct Answer {
  mpe_result r;
  std::vector<uint32_t> match;
  mpe_rig_init_info info;
};
Answer run(const Problem& P, int chunk = 0, int min_rows = 6, int min_markers = 4, int min_margin = 1) {
  Answer a;
  std::memset(&a.r, 0xff, sizeof(a.r));
  std::memset(&a.info, 0xff, sizeof(a.info));
  a.match.assign((size_t)P.n_cam * P.n_mk, 0xffffffffu);
  host_rig_init_chunked(P.cams.data(), P.n_cam, P.mk.data(), P.n_mk, P.beg.data(), P.det.data(), P.tol.data(), P.tol.data(), 2,
                        min_rows, min_markers, min_margin, chunk, &a.r, a.match.data(), &a.info);
  return a;
}
bool identity_and_zero(const mpe_result& r) {
  bool ok = r.status == MPE_FRAME_NO_POSE;
  for (int i = 0; i < 16; ++i) ok = ok && r.T[i] == (i % 5 == 0 ? 1.0 : 0.0);
  for (int i = 0; i < 36; ++i) ok = ok && r.cov[i] == 0.0;
  return ok;
}
}  // namespace

int main() {
  std::mt19937 g(20261020);
  // ---- the unranking against nested loops: three cameras with 5, 2 and 4 detections, 4 markers
  long n_decoded = 0;
  {
    const int n_det[3] = {5, 2, 4}, n_mk = 4;
    int item = 0;
    for (int c = 0; c < 3; ++c)
      for (int i = 0; i < n_det[c]; ++i)
        for (int j = i + 1; j < n_det[c]; ++j)
          for (int k = j + 1; k < n_det[c]; ++k)
            for (int a = 0; a < n_mk; ++a)
              for (int b = 0; b < n_mk; ++b)
                for (int d = 0; d < n_mk; ++d) {
                  if (a == b || a == d || b == d) continue;
                  int got[7];
                  host_rig_init_decode(n_det, 3, n_mk, item, got);
                  const int want[7] = {c, i, j, k, a, b, d};
                  CHECK(std::memcmp(got, want, sizeof(want)) == 0, "item %d: (%d; %d %d %d; %d %d %d)", item, got[0], got[1], got[2],
                        got[3], got[4], got[5], got[6]);
                  ++item, ++n_decoded;
                }
    CHECK(item == (10 + 0 + 4) * 24, "%d items", item);
  }
  // ---- a body spread over the cameras, no camera with four LEDs
  long n_rigs = 0, n_none = 0;
  for (int it = 0; it < 12; ++it) {
    const int n_cam = 2 + it % 3, n_mk = 5;
    std::vector<int> first(n_cam), seen(n_cam), stray(n_cam);
    for (int c = 0; c < n_cam; ++c) {
      first[c] = (2 * c) % n_mk;
      seen[c] = c == n_cam - 1 && n_cam > 2 ? 2 : 3;
      stray[c] = (int)(g() % 3);
    }
    if (n_cam == 2) first[1] = 2, seen[0] = seen[1] = 3;  // {0, 1, 2} and {2, 3, 4}: six rows, five markers
    const Problem P = make(g, n_cam, n_mk, first, seen, stray);
    const Answer a = run(P);
    double worst = 0;
    for (int i = 0; i < 16; ++i) worst = std::fmax(worst, std::fabs(a.r.T[i] - P.T_true.a[i]));
    CHECK(a.info.best_rows == P.n_seen_rows, "rig %d: %d rows of %d", it, a.info.best_rows, P.n_seen_rows);
    CHECK(a.info.reason == 0 || a.info.reason == 5, "rig %d: reason %d (rows %d, runner %d)", it, a.info.reason, a.info.best_rows,
          a.info.runner_rows);
    if (a.info.reason == 0) {
      CHECK(a.r.status == MPE_FRAME_POSE && worst < 1e-8, "rig %d: status %d, %.3g off", it, a.r.status, worst);
      CHECK(a.r.n_corr == P.n_seen_rows && a.info.track.rows == P.n_seen_rows, "rig %d: %d rows", it, a.r.n_corr);
    } else {
      CHECK(identity_and_zero(a.r) && a.info.runner_rows == a.info.best_rows, "rig %d: an ambiguous record", it);
      ++n_none;
    }
    // the same bits whatever the chunk
    for (int chunk : {1, 7, 100000}) {
      const Answer b = run(P, chunk);
      CHECK(std::memcmp(&a.r, &b.r, sizeof(a.r)) == 0 && std::memcmp(&a.info, &b.info, sizeof(a.info)) == 0 && a.match == b.match,
            "rig %d: chunk %d changes the result", it, chunk);
    }
    ++n_rigs;
  }
  // ---- no pose
  {
    const Problem P = make(g, 1, 5, {0}, {3}, {0});  // three rows: reason 1
    const Answer a = run(P);
    CHECK(a.info.reason == 1 && a.info.best_rows == 3 && a.info.n_items == 60 && identity_and_zero(a.r), "three rows: reason %d",
          a.info.reason);
    CHECK(a.r.n_corr == 3 && a.r.n_det == 1 && a.info.track.rounds == 0, "three rows: n_corr %d", a.r.n_corr);
    ++n_none;
    const Problem Q = make(g, 16, 5, std::vector<int>(16, 0), std::vector<int>(16, 2), std::vector<int>(16, 0));  // no item: 6
    const Answer b = run(Q);
    CHECK(b.info.reason == 6 && b.info.n_items == 0 && b.info.camera == -1 && identity_and_zero(b.r), "16 x 2: reason %d",
          b.info.reason);
    for (uint32_t w : b.match) CHECK(w == 0, "16 x 2: a match word");
    ++n_none;
    const Problem R = make(g, 3, 5, {0, 0, 0}, {0, 0, 0}, {5, 5, 5});  // clutter alone
    const Answer c = run(R);
    CHECK(c.info.reason != 0 && identity_and_zero(c.r) && c.info.n_items == 3 * 10 * 60, "clutter: reason %d", c.info.reason);
    ++n_none;
  }
  if (g_failed) {
    std::printf("rig_init_host: %d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("rig_init_host ok: %ld items decoded, %ld rigs, %ld without a pose, LDS %d bytes\n", n_decoded, n_rigs, n_none,
              (int)sizeof(RigInitLds));
  return 0;
}
#endif
