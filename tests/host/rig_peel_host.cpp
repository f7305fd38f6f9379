// rig_peel_host.cpp — several bodies in one frame on the host (test scaffolding, CPU tier): the peel step between the
// rounds (csrc/mpe_rig_peel.h, as it is) around the host form of the rig initialiser's four steps (csrc/mpe_rig_init.h
// behind the same cut-outs tests/host/rig_init_host.cpp stands on).  host_rig_bodies runs ONE problem the way
// mpe_rig_init_bodies_batch runs it on the device: per round the count step (a loop over the 64 lanes of every list
// where the device has a wave and a __ballot), the scan, the scatter, then vote / winner / runner-up / finish over the
// compacted lists with as many voting blocks as the HOST counted — from the lists claimed_in leaves (blocks = 0, the
// device's way: an upper bound) or from the round's own lists (blocks = 1, the exact count) —, and behind the last round
// the count step once more.  Two uses: a shared library for tests/test_rig_bodies_host.py, and — with
// -DRIG_PEEL_HOST_MAIN — a stand-alone program that the test builds plain and under -fsanitize=address,undefined: scenes
// of two and three bodies among stray points, a list of 64 with its first and last point claimed, a body that is not
// asked for, and both block counts.  Prints "rig_peel_host ok: ..." and returns 0, or says what failed and returns 1.
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
#include "mpe_rig_peel.h"
namespace mpe {
#include "k2_head_extract.inc"
#include "k3_extract.inc"
#include "mpe_rig_gn.h"
#include "mpe_rig_track.h"
#include "mpe_rig_init.h"
}  // namespace mpe
using namespace mpe;

namespace {
// one round over the lists det_begin / det_xy in n_blocks voting blocks of MPE_RIG_INIT_CHUNK items (k_rig_init_vote,
// k_rig_init_winner, k_rig_init_vote against the winner, k_rig_init_finish)
void host_round(const mpe_rig_camera* cams, int n_cam, const double* markers, int n_mk, const int* det_begin,
                const double* det_xy, const double* tol_vote, const double* tol_accept, const mpe_rig_init_options& o,
                int n_blocks, mpe_result* out, uint32_t* match, mpe_rig_init_info* info) {
  RigInitLds* S = new RigInitLds;
  unsigned char W[MPE_RIG_MAX_ROWS];
  rig_init_stage(*S, 0, 1, cams, n_cam, markers, n_mk, det_begin, det_xy, tol_vote, nullptr);
  const int n_items = S->off[n_cam] < MPE_RIG_INIT_MAX_ITEMS ? S->off[n_cam] : MPE_RIG_INIT_MAX_ITEMS;
  std::vector<RigInitKey> keys((size_t)n_blocks);
  int unused = 0;
  for (int blk = 0; blk < n_blocks; ++blk) {
    RigInitKey key = rig_init_no_key();
    const long long first = (long long)blk * MPE_RIG_INIT_CHUNK;
    for (long long item = first; item < n_items && item < first + MPE_RIG_INIT_CHUNK; ++item)
      rig_init_item(*S, 0, n_cam, n_mk, (int)item, 0, key, unused);
    keys[(size_t)blk] = key;
  }
  RigInitKey win = rig_init_no_key();
  for (const RigInitKey& k : keys)
    if (rig_init_better(k, win)) win = k;
  rig_init_winner(*S, 0, n_cam, n_mk, win, W, info);
  int runner = 0;
  if (win.h >= 0) {
    rig_init_stage(*S, 0, 1, cams, n_cam, markers, n_mk, det_begin, det_xy, tol_vote, W);
    for (int blk = 0; blk < n_blocks; ++blk) {
      RigInitKey none = rig_init_no_key();
      int r = 0;
      const long long first = (long long)blk * MPE_RIG_INIT_CHUNK;
      for (long long item = first; item < n_items && item < first + MPE_RIG_INIT_CHUNK; ++item)
        rig_init_item(*S, 0, n_cam, n_mk, (int)item, 1, none, r);
      runner = r > runner ? r : runner;
    }
  }
  delete S;
  RigTrackLds* T = new RigTrackLds;
  rig_init_finish(*T, cams, n_cam, markers, n_mk, det_begin, det_xy, tol_vote, tol_accept, W, runner, o.max_rounds, o.min_rows,
                  o.min_markers, o.min_margin, out, match, info);
  delete T;
}

int blocks_of(const int* n_per_list, int n_cam, int n_mk) {
  long long items = 0;
  for (int c = 0; c < n_cam; ++c) items += rig_init_camera_items(n_per_list[c] < MPE_MAX_DETECTIONS ? n_per_list[c] : MPE_MAX_DETECTIONS, n_mk);
  return (int)((items + MPE_RIG_INIT_CHUNK - 1) / MPE_RIG_INIT_CHUNK);
}
}  // namespace

// ONE problem.  markers: the bodies' marker sets one behind the other, n_mk[b] x 3 each; options: n_bodies records;
// det_begin: n_cam + 1 entries from 0; claimed_in / find: optional.  blocks: 0 the device's count (from the lists
// claimed_in leaves), 1 the exact count of every round.  out / info: n_bodies, match: n_bodies x n_cam x MPE_MAX_MARKERS,
// owner: a byte per point.
extern "C" void host_rig_bodies(const mpe_rig_camera* cams, int n_cam, const double* markers, const int* n_mk,
                                const mpe_rig_init_options* options, int n_bodies, const int* det_begin, const double* det_xy,
                                const uint8_t* claimed_in, const uint8_t* find, const double* tol_vote, const double* tol_accept,
                                int blocks, mpe_result* out, uint32_t* match, mpe_rig_init_info* info, int8_t* owner) {
  const int n_det = det_begin[n_cam];
  std::vector<int> counts((size_t)n_cam), r_begin((size_t)n_cam + 1, 0), map((size_t)n_det + 1), left((size_t)n_cam, 0);
  std::vector<double> r_xy(2 * (size_t)n_det + 2);
  std::vector<uint32_t> r_match((size_t)n_cam * MPE_MAX_MARKERS, 0);
  mpe_result r_out;
  mpe_rig_init_info r_info;
  std::memset(&r_out, 0, sizeof(r_out));
  std::memset(&r_info, 0, sizeof(r_info));
  for (int k = 0; k < n_det; ++k) owner[k] = (claimed_in && claimed_in[k]) ? MPE_RIG_PEEL_TAKEN : MPE_RIG_PEEL_FREE;
  for (int c = 0; c < n_cam; ++c)
    for (int k = det_begin[c]; k < det_begin[c + 1]; ++k) left[(size_t)c] += owner[k] == MPE_RIG_PEEL_FREE ? 1 : 0;
  const double* mk = markers;
  for (int round = 0; round <= n_bodies; ++round) {
    // ---- k_rig_peel_count
    const int n_mk_prev = round > 0 ? n_mk[round - 1] : 0;
    const bool asked_prev = round > 0 && (!find || find[round - 1] != 0);
    const bool asked = round < n_bodies && (!find || find[round] != 0);
    for (int c = 0; c < n_cam; ++c) {
      const int b0 = det_begin[c], n = det_begin[c + 1] - b0;
      uint64_t mask = 0;
      for (int j = 0; j < 64; ++j) {
        int8_t own = j < n ? owner[b0 + j] : (int8_t)MPE_RIG_PEEL_TAKEN;
        if (asked_prev)
          own = rig_peel_fold(own, j, r_info.reason == 0, &r_match[(size_t)c * n_mk_prev], n_mk_prev, &map[(size_t)r_begin[(size_t)c]],
                              round - 1);
        if (j < n) owner[b0 + j] = own;
        if (asked && j < n && own == MPE_RIG_PEEL_FREE) mask |= (uint64_t)1 << j;
      }
      counts[(size_t)c] = rig_peel_count(mask);
    }
    if (round > 0) {
      const int pb = round - 1;
      for (int c = 0; c < n_cam; ++c)
        for (int m = 0; m < MPE_MAX_MARKERS; ++m)
          match[((size_t)pb * n_cam + c) * MPE_MAX_MARKERS + m] =
              (asked_prev && m < n_mk_prev) ? rig_peel_word(r_match[(size_t)c * n_mk_prev + m], &map[(size_t)r_begin[(size_t)c]]) : 0u;
      if (asked_prev) {
        out[pb] = r_out;
        rig_peel_info(r_info, r_info.camera >= 0 ? &map[(size_t)r_begin[(size_t)r_info.camera]] : nullptr, &info[pb]);
      } else {
        rig_peel_not_asked(&out[pb], &info[pb]);
      }
    }
    if (round == n_bodies) break;
    // ---- k_rig_peel_scan, k_rig_peel_scatter
    for (int c = 0; c < n_cam; ++c) r_begin[(size_t)c + 1] = r_begin[(size_t)c] + counts[(size_t)c];
    for (int c = 0; c < n_cam; ++c) {
      const int b0 = det_begin[c], n = det_begin[c + 1] - b0;
      uint64_t mask = 0;
      for (int j = 0; j < n; ++j)
        if (asked && owner[b0 + j] == MPE_RIG_PEEL_FREE) mask |= (uint64_t)1 << j;
      for (int j = 0; j < n; ++j)
        if ((mask >> j) & 1u) {
          const size_t at = (size_t)r_begin[(size_t)c] + (size_t)rig_peel_position(mask, j);
          r_xy[2 * at] = det_xy[2 * (size_t)(b0 + j)];
          r_xy[2 * at + 1] = det_xy[2 * (size_t)(b0 + j) + 1];
          map[at] = j;
        }
    }
    // ---- the round
    const int n_blocks = !asked ? 0 : blocks != 0 ? blocks_of(counts.data(), n_cam, n_mk[round]) : blocks_of(left.data(), n_cam, n_mk[round]);
    std::fill(r_match.begin(), r_match.end(), 0xffffffffu);
    host_round(cams, n_cam, mk, n_mk[round], r_begin.data(), r_xy.data(), tol_vote, tol_accept, options[round], n_blocks, &r_out,
               r_match.data(), &r_info);
    mk += 3 * (size_t)n_mk[round];
  }
}

// the single-body run over given lists (what a round must equal over the host-filtered lists), exact block count
extern "C" void host_rig_single(const mpe_rig_camera* cams, int n_cam, const double* markers, int n_mk,
                                const mpe_rig_init_options* o, const int* det_begin, const double* det_xy, const double* tol_vote,
                                const double* tol_accept, mpe_result* out, uint32_t* match, mpe_rig_init_info* info) {
  std::vector<int> n((size_t)n_cam);
  for (int c = 0; c < n_cam; ++c) n[(size_t)c] = det_begin[c + 1] - det_begin[c];
  host_round(cams, n_cam, markers, n_mk, det_begin, det_xy, tol_vote, tol_accept, *o, blocks_of(n.data(), n_cam, n_mk), out, match,
             info);
}

#ifdef RIG_PEEL_HOST_MAIN
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

const double M5[15] = {0.0714197, 0.0800214, 0.0622611, 0.0400755, -0.0912328, 0.0317064, -0.0647293, -0.0879977,
                       0.0830852, -0.0558663, -0.0165446, 0.053473, 0.0120, 0.0310, 0.1210};

struct Scene {
  mpe_rig_camera cam;
  std::vector<double> det;     // the list
  std::vector<int> truth;      // per point: the body it belongs to, -1 a stray point
  std::vector<double> T_true;  // per body 16
  int n_bodies;
};
// n_bodies copies of M5 in front of one camera (exact pixels, blobs at least 12 px apart), n_stray stray points, shuffled
Scene make(std::mt19937& g, int n_bodies, int n_stray) {
  std::uniform_real_distribution<double> ud(0.0, 1.0);
  std::normal_distribution<double> nd;
  Scene s;
  s.n_bodies = n_bodies;
  std::memset(&s.cam, 0, sizeof(s.cam));
  s.cam.K[0] = 615.65, s.cam.K[4] = 616.76, s.cam.K[2] = 362.66, s.cam.K[5] = 256.67, s.cam.K[8] = 1;
  for (int i = 0; i < 16; i += 5) s.cam.T_cam_rig[i] = 1.0;
  std::vector<double> pts;
  std::vector<int> who;
  auto far_from_all = [&](double x, double y, double sep) {
    for (size_t k = 0; k < who.size(); ++k)
      if (std::hypot(x - pts[2 * k], y - pts[2 * k + 1]) < sep) return false;
    return true;
  };
  for (int b = 0; b < n_bodies;) {
    double ax[3] = {nd(g), nd(g), nd(g)};
    const double nrm = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    const double th = 0.8 * ud(g), sn = std::sin(th), cs = std::cos(th);
    for (double& v : ax) v /= nrm;
    const double Kx[3][3] = {{0, -ax[2], ax[1]}, {ax[2], 0, -ax[0]}, {-ax[1], ax[0], 0}};
    double T[16] = {0};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double k2 = 0;
        for (int k = 0; k < 3; ++k) k2 += Kx[i][k] * Kx[k][j];
        T[4 * i + j] = (i == j ? 1.0 : 0.0) + sn * Kx[i][j] + (1 - cs) * k2;
      }
    T[3] = 0.6 * ud(g) - 0.3, T[7] = 0.4 * ud(g) - 0.2, T[11] = 0.8 + 1.7 * ud(g), T[15] = 1;
    double px[10];
    bool ok = true;
    for (int m = 0; m < 5 && ok; ++m) {
      double q[3];
      for (int i = 0; i < 3; ++i) q[i] = T[4 * i] * M5[3 * m] + T[4 * i + 1] * M5[3 * m + 1] + T[4 * i + 2] * M5[3 * m + 2] + T[4 * i + 3];
      px[2 * m] = s.cam.K[0] * q[0] / q[2] + s.cam.K[2];
      px[2 * m + 1] = s.cam.K[4] * q[1] / q[2] + s.cam.K[5];
      ok = px[2 * m] > 12 && px[2 * m] < 740 && px[2 * m + 1] > 12 && px[2 * m + 1] < 468 && far_from_all(px[2 * m], px[2 * m + 1], 12.0);
      for (int k = 0; k < m && ok; ++k) ok = std::hypot(px[2 * m] - px[2 * k], px[2 * m + 1] - px[2 * k + 1]) >= 12.0;
    }
    if (!ok) continue;
    for (int m = 0; m < 5; ++m) pts.push_back(px[2 * m]), pts.push_back(px[2 * m + 1]), who.push_back(b);
    s.T_true.insert(s.T_true.end(), T, T + 16);
    ++b;
  }
  for (int k = 0; k < n_stray;) {
    const double x = 12 + 728 * ud(g), y = 12 + 456 * ud(g);
    if (!far_from_all(x, y, 12.0)) continue;
    pts.push_back(x), pts.push_back(y), who.push_back(-1);
    ++k;
  }
  std::vector<int> order(who.size());
  for (size_t k = 0; k < order.size(); ++k) order[k] = (int)k;
  std::shuffle(order.begin(), order.end(), g);
  for (int k : order) s.det.push_back(pts[2 * (size_t)k]), s.det.push_back(pts[2 * (size_t)k + 1]), s.truth.push_back(who[(size_t)k]);
  return s;
}

struct Answer {
  std::vector<mpe_result> r;
  std::vector<uint32_t> match;
  std::vector<mpe_rig_init_info> info;
  std::vector<int8_t> owner;
};
Answer run(const Scene& s, int n_ask, const uint8_t* claimed, const uint8_t* find, int blocks) {
  Answer a;
  a.r.resize((size_t)n_ask);
  a.info.resize((size_t)n_ask);
  a.match.assign((size_t)n_ask * MPE_MAX_MARKERS, 0xffffffffu);
  a.owner.assign(s.truth.size(), 99);
  std::memset(a.r.data(), 0xff, a.r.size() * sizeof(mpe_result));
  std::memset(a.info.data(), 0xff, a.info.size() * sizeof(mpe_rig_init_info));
  std::vector<double> mk;
  std::vector<int> n_mk((size_t)n_ask, 5);
  std::vector<mpe_rig_init_options> opt((size_t)n_ask, mpe_rig_init_options{2, 5, 5, 0});
  for (int b = 0; b < n_ask; ++b) mk.insert(mk.end(), M5, M5 + 15);
  const int beg[2] = {0, (int)s.truth.size()};
  const double tol = 3.0;
  host_rig_bodies(&s.cam, 1, mk.data(), n_mk.data(), opt.data(), n_ask, beg, s.det.data(), claimed, find, &tol, &tol, blocks,
                  a.r.data(), a.match.data(), a.info.data(), a.owner.data());
  return a;
}
bool same(const Answer& a, const Answer& b) {
  return a.match == b.match && a.owner == b.owner && std::memcmp(a.r.data(), b.r.data(), a.r.size() * sizeof(mpe_result)) == 0 &&
         std::memcmp(a.info.data(), b.info.data(), a.info.size() * sizeof(mpe_rig_init_info)) == 0;
}
// which true body a pose is: the one whose translation is within 2 cm, -1 none
int body_of(const Scene& s, const mpe_result& r) {
  for (int b = 0; b < s.n_bodies; ++b) {
    const double* T = &s.T_true[16 * (size_t)b];
    if (std::hypot(std::hypot(r.T[3] - T[3], r.T[7] - T[7]), r.T[11] - T[11]) < 0.02) return b;
  }
  return -1;
}
}  // namespace

int main() {
  std::mt19937 g(20261021);
  long n_scenes = 0, n_found = 0;
  // ---- two and three identical bodies among stray points; one body more than is in view
  for (int it = 0; it < 8; ++it) {
    const int n_true = 2 + it % 2, n_stray = 2 * (it % 3);
    const Scene s = make(g, n_true, n_stray);
    const Answer a = run(s, n_true + 1, nullptr, nullptr, 0);
    unsigned seen = 0;
    for (int b = 0; b < n_true; ++b) {
      const int t = a.r[(size_t)b].status == MPE_FRAME_POSE ? body_of(s, a.r[(size_t)b]) : -1;
      CHECK(t >= 0 && !(seen & (1u << t)), "scene %d body %d: status %d reason %d true body %d", it, b, a.r[(size_t)b].status,
            a.info[(size_t)b].reason, t);
      if (t < 0) continue;
      seen |= 1u << t;
      ++n_found;
      for (size_t k = 0; k < s.truth.size(); ++k)
        CHECK((a.owner[k] == b) == (s.truth[k] == t), "scene %d body %d: point %d owner %d truth %d", it, b, (int)k, a.owner[k], s.truth[k]);
      for (int m = 0; m < MPE_MAX_MARKERS; ++m) {
        const uint32_t w = a.match[(size_t)b * MPE_MAX_MARKERS + m];
        CHECK(m < 5 ? (w >= 1 && w <= s.truth.size() && s.truth[w - 1] == t) : w == 0, "scene %d body %d marker %d: word %u", it, b, m, w);
      }
    }
    CHECK(a.r[(size_t)n_true].status == MPE_FRAME_NO_POSE && a.info[(size_t)n_true].reason != 0, "scene %d: the absent body has a pose", it);
    for (size_t k = 0; k < s.truth.size(); ++k) CHECK(a.owner[k] != n_true, "scene %d: the absent body owns point %d", it, (int)k);
    CHECK(same(a, run(s, n_true + 1, nullptr, nullptr, 1)), "scene %d: the block count shows", it);
    ++n_scenes;
  }
  // ---- a body that is not asked for claims nothing and answers "not asked"
  {
    const Scene s = make(g, 2, 3);
    const uint8_t find[3] = {1, 0, 1};
    const Answer a = run(s, 3, nullptr, find, 0);
    CHECK(a.info[1].reason == MPE_RIG_PEEL_NOT_ASKED && a.r[1].status == MPE_FRAME_NO_POSE && a.r[1].T[0] == 1.0 && a.r[1].T[1] == 0.0 &&
              a.r[1].n_det == 0 && a.info[1].n_items == 0,
          "not asked: reason %d", a.info[1].reason);
    for (int m = 0; m < MPE_MAX_MARKERS; ++m) CHECK(a.match[MPE_MAX_MARKERS + m] == 0, "not asked: a match word");
    CHECK(a.r[0].status == MPE_FRAME_POSE && a.r[2].status == MPE_FRAME_POSE && body_of(s, a.r[0]) != body_of(s, a.r[2]), "find 1 0 1");
    for (size_t k = 0; k < s.truth.size(); ++k) CHECK(a.owner[k] != 1 && (a.owner[k] == -1) == (s.truth[k] < 0), "find 1 0 1: owner %d", a.owner[k]);
    ++n_scenes;
  }
  // ---- a list of 64 of which claimed_in takes index 0 and index 63 (4 markers: 238 266 items of 62 points)
  {
    Scene s = make(g, 1, 59);
    CHECK(s.truth.size() == 64, "%d points", (int)s.truth.size());
    for (size_t k = 1; k < 63; ++k)  // keep the body away from both ends
      for (size_t e : {(size_t)0, (size_t)63})
        if (s.truth[e] == 0 && s.truth[k] < 0) {
          std::swap(s.truth[e], s.truth[k]);
          std::swap(s.det[2 * e], s.det[2 * k]);
          std::swap(s.det[2 * e + 1], s.det[2 * k + 1]);
        }
    std::vector<uint8_t> claimed(64, 0);
    claimed[0] = claimed[63] = 1;
    Answer a;
    a.r.resize(1), a.info.resize(1), a.match.assign(MPE_MAX_MARKERS, 0xffffffffu), a.owner.assign(64, 99);
    const int n_mk = 4, beg[2] = {0, 64};
    const mpe_rig_init_options opt = {2, 4, 4, 0};
    const double tol = 1.0;
    host_rig_bodies(&s.cam, 1, M5, &n_mk, &opt, 1, beg, s.det.data(), claimed.data(), nullptr, &tol, &tol, 0, a.r.data(),
                    a.match.data(), a.info.data(), a.owner.data());
    CHECK(a.info[0].n_items == 62LL * 61 * 60 / 6 * 24, "items %lld", (long long)a.info[0].n_items);
    CHECK(a.owner[0] == -2 && a.owner[63] == -2, "owner of the claimed ends %d %d", a.owner[0], a.owner[63]);
    CHECK(a.r[0].status == MPE_FRAME_POSE && body_of(s, a.r[0]) == 0, "list of 64: status %d reason %d", a.r[0].status, a.info[0].reason);
    for (int m = 0; m < 4; ++m) {
      const uint32_t w = a.match[(size_t)m];
      CHECK(w >= 2 && w <= 63 && s.truth[w - 1] == 0 && a.owner[w - 1] == 0, "list of 64: marker %d word %u", m, w);
    }
    ++n_scenes;
  }
  if (g_failed) {
    std::printf("rig_peel_host: %d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("rig_peel_host ok: %ld scenes, %ld bodies found\n", n_scenes, n_found);
  return 0;
}
#endif
