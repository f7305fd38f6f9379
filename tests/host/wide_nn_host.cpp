// wide_nn_host.cpp — the logic of k_nn_wide (csrc/mpe_wide_nn.h) as a stand-alone host program: the 64-lane form (every
// lane reduces its four detections with wide_nn_lane, the wave reduces the pairs by the butterfly of the kernel with
// wide_nn_better) is emulated lane by lane and compared with the plain double loop of findCorrespondences written out
// here, for random sets of 0 .. 256 detections and 1 .. 16 markers, exact ties (the equal minimum in different lanes and
// in the same lane), predictions exactly nn_tol away, NaN predictions and NaN detections, and two markers naming one
// detection; the compaction (wide_hand_over) is compared with the rows it was made from.  Built plain and with
// -fsanitize=address,undefined (tools/host_sanitize.sh); prints "wide_nn_host ok: ..." and returns 0, or says what failed
// and returns 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "mpe_wide_nn.h"

namespace {
int g_failed = 0;
long long g_sets = 0, g_rows = 0, g_ties = 0, g_shared = 0, g_edge_kept = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      std::printf("FAILED %s: ", #cond); \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
      ++g_failed;                        \
    }                                    \
  } while (0)

// findCorrespondences as the narrow tracked path spells it (first strict minimum over ascending j)
int plain_rows(const double* pred, int n_m, const double* det, int n_d, double tol, unsigned* cm, unsigned* cd) {
  int n_c = 0;
  for (int i = 0; i < n_m; ++i) {
    double best = std::numeric_limits<double>::infinity();
    unsigned bj = 0;
    for (int j = 0; j < n_d; ++j) {
      const double du = pred[2 * i] - det[2 * j], dv = pred[2 * i + 1] - det[2 * j + 1];
      const double d2 = du * du + dv * dv;
      if (d2 < best) {
        best = d2;
        bj = (unsigned)j + 1;
      }
    }
    if (bj != 0 && std::sqrt(best) <= tol) {
      cm[n_c] = (unsigned)i + 1;
      cd[n_c] = bj;
      ++n_c;
    }
  }
  return n_c;
}

// the wave of k_nn_wide, lane by lane
int lane_rows(const double* pred, int n_m, const double* det, int n_d, double tol, unsigned* cm, unsigned* cd) {
  double lx[64][MPE_WIDE_NN_PER_LANE], ly[64][MPE_WIDE_NN_PER_LANE];
  for (int l = 0; l < 64; ++l)
    for (int k = 0; k < MPE_WIDE_NN_PER_LANE; ++k) {
      const int j = l + 64 * k;
      lx[l][k] = j < n_d ? det[2 * j] : 0.0;
      ly[l][k] = j < n_d ? det[2 * j + 1] : 0.0;
    }
  int n_c = 0;
  for (int i = 0; i < n_m; ++i) {
    double best[64], nb[64];
    unsigned bj[64], nj[64];
    for (int l = 0; l < 64; ++l) mpe::wide_nn_lane(lx[l], ly[l], l, n_d, pred[2 * i], pred[2 * i + 1], best[l], bj[l]);
    for (int m = 1; m < 64; m <<= 1) {
      for (int l = 0; l < 64; ++l) {
        const bool take = mpe::wide_nn_better(best[l ^ m], bj[l ^ m], best[l], bj[l]);
        nb[l] = take ? best[l ^ m] : best[l];
        nj[l] = take ? bj[l ^ m] : bj[l];
      }
      std::memcpy(best, nb, sizeof(best));
      std::memcpy(bj, nj, sizeof(bj));
    }
    for (int l = 1; l < 64; ++l)
      CHECK(bj[l] == bj[0] && (best[l] == best[0] || (best[l] != best[l] && best[0] != best[0])), "lane %d disagrees with lane 0", l);
    if (mpe::wide_nn_keep(best[0], bj[0], tol)) {
      cm[n_c] = (unsigned)i + 1;
      cd[n_c] = bj[0];
      ++n_c;
    }
  }
  return n_c;
}

void check_set(const std::vector<double>& pred, int n_m, const std::vector<double>& det, int n_d, double tol, const char* what) {
  unsigned cm0[MPE_MAX_MARKERS], cd0[MPE_MAX_MARKERS], cm1[MPE_MAX_MARKERS], cd1[MPE_MAX_MARKERS], cm2[MPE_MAX_MARKERS],
      cd2[MPE_MAX_MARKERS];
  const int n0 = plain_rows(pred.data(), n_m, det.data(), n_d, tol, cm0, cd0);
  const int n1 = lane_rows(pred.data(), n_m, det.data(), n_d, tol, cm1, cd1);
  const int n2 = mpe::wide_nn_rows(pred.data(), n_m, det.data(), n_d, tol, cm2, cd2);
  CHECK(n0 == n1 && n0 == n2, "%s: %d rows plain, %d lanes, %d sequential (n_d %d, n_m %d)", what, n0, n1, n2, n_d, n_m);
  for (int r = 0; r < n0 && r < n1 && r < n2; ++r)
    CHECK(cm0[r] == cm1[r] && cd0[r] == cd1[r] && cm0[r] == cm2[r] && cd0[r] == cd2[r],
          "%s: row %d plain (%u, %u) lanes (%u, %u) sequential (%u, %u)", what, r, cm0[r], cd0[r], cm1[r], cd1[r], cm2[r], cd2[r]);
  ++g_sets;
  g_rows += n0;
  // the hand-over against the rows it was made from
  mpe_detections_wide w;
  std::memset(&w, 0, sizeof(w));
  w.n = n_d;
  for (int j = 0; j < n_d; ++j) {
    w.undist_xy[2 * j] = det[2 * j];
    w.undist_xy[2 * j + 1] = det[2 * j + 1];
    w.dist_xy[2 * j] = (float)(1000 + j);
    w.dist_xy[2 * j + 1] = (float)(2000 + j);
  }
  mpe_detections o;
  std::memset(&o, 0xff, sizeof(o));
  uint32_t cc[2 * MPE_MAX_MARKERS], sw[MPE_MAX_MARKERS];
  mpe::wide_hand_over(&w, cm1, cd1, n1, &o, cc, sw);
  int distinct = 0;
  for (int r = 0; r < n1; ++r) {
    bool seen = false;
    for (int q = 0; q < r; ++q) seen |= cd1[q] == cd1[r];
    distinct += seen ? 0 : 1;
  }
  g_shared += n1 - distinct;
  CHECK(o.n == (distinct == 0 ? 0 : (distinct < 4 ? 4 : distinct)), "%s: compact n %d for %d distinct", what, o.n, distinct);
  CHECK(o.status == 0, "%s: status %d", what, o.status);
  for (int r = 0; r < MPE_MAX_MARKERS; ++r) {
    if (r >= n1) {
      CHECK(cc[2 * r] == 0 && cc[2 * r + 1] == 0, "%s: row %d beyond the rows is not empty", what, r);
      continue;
    }
    const unsigned s = cc[2 * r + 1];
    CHECK(cc[2 * r] == cm1[r] && s >= 1 && (int)s <= distinct, "%s: compact row %d = (%u, %u)", what, r, cc[2 * r], s);
    if (s < 1 || (int)s > distinct) continue;
    CHECK(sw[s - 1] == cd1[r], "%s: slot %u is wide %u, row names %u", what, s, sw[s - 1], cd1[r]);
    const int j = (int)cd1[r] - 1;
    const bool same = !std::memcmp(&o.undist_xy[2 * (s - 1)], &w.undist_xy[2 * j], 2 * sizeof(double)) &&
                      o.dist_xy[2 * (s - 1)] == w.dist_xy[2 * j] && o.dist_xy[2 * (s - 1) + 1] == w.dist_xy[2 * j + 1];
    CHECK(same, "%s: slot %u does not hold detection %d", what, s, j + 1);
  }
  for (int k = 0; k < MPE_MAX_MARKERS; ++k) {
    if (k < distinct) {
      CHECK(sw[k] >= 1 && (int)sw[k] <= n_d && (k == 0 || sw[k] > sw[k - 1]), "%s: slot table not ascending at %d", what, k);
    } else {
      CHECK(sw[k] == 0, "%s: slot %d beyond the slots = %u", what, k, sw[k]);
    }
  }
  for (int k = distinct; k < o.n; ++k)  // padding: copies of the first slot
    CHECK(!std::memcmp(&o.undist_xy[2 * k], &o.undist_xy[0], 2 * sizeof(double)), "%s: pad slot %d", what, k);
}
}  // namespace

int main() {
  const int sizes[] = {0, 1, 3, 4, 63, 64, 65, 128, 255, 256};
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::mt19937_64 rng(20260419);
  std::uniform_real_distribution<double> ux(0.0, 752.0), uy(0.0, 480.0), jit(-4.0, 4.0);
  for (int n_d : sizes)
    for (int n_m = 1; n_m <= MPE_MAX_MARKERS; ++n_m)
      for (int rep = 0; rep < 6; ++rep) {
        std::vector<double> det((size_t)2 * (n_d > 0 ? n_d : 1)), pred((size_t)2 * n_m);
        for (int j = 0; j < n_d; ++j) {
          det[2 * j] = ux(rng);
          det[2 * j + 1] = uy(rng);
        }
        // predictions: near a detection (most are kept), sometimes two markers near the same one, sometimes far away
        for (int i = 0; i < n_m; ++i) {
          if (n_d > 0 && rep != 5) {
            const int j = (rep == 1 && i > 0) ? (int)(rng() % (unsigned)((i + 1) / 2 + 1)) % n_d : (int)(rng() % (unsigned)n_d);
            pred[2 * i] = det[2 * j] + jit(rng);
            pred[2 * i + 1] = det[2 * j + 1] + jit(rng);
          } else {
            pred[2 * i] = ux(rng);
            pred[2 * i + 1] = uy(rng);
          }
        }
        check_set(pred, n_m, det, n_d, 5.0, "random");
        // exact ties: detection a copied to another lane (a + 1) and to the same lane (a + 64), in both directions
        if (n_d >= 2) {
          std::vector<double> dt = det;
          const int a = (int)(rng() % (unsigned)(n_d - 1));
          const int far = a + 64 < n_d ? a + 64 : -1;
          dt[2 * (a + 1)] = dt[2 * a];
          dt[2 * (a + 1) + 1] = dt[2 * a + 1];
          if (far >= 0) {
            dt[2 * far] = dt[2 * a];
            dt[2 * far + 1] = dt[2 * a + 1];
          }
          std::vector<double> pt = pred;
          pt[0] = dt[2 * a] + 0.5;
          pt[1] = dt[2 * a + 1] - 0.25;
          unsigned cm[MPE_MAX_MARKERS], cd[MPE_MAX_MARKERS];
          const int nc = plain_rows(pt.data(), n_m, dt.data(), n_d, 5.0, cm, cd);
          CHECK(nc >= 1 && cm[0] == 1 && (int)cd[0] <= a + 1, "tie: marker 1 names %u, the copies start at %d", nc ? cd[0] : 0, a + 1);
          check_set(pt, n_m, dt, n_d, 5.0, "tie");
          ++g_ties;
          // ... and with the LAST copy the one in the low lane: a tie between lane a + 1 (index a + 2) and lane a
          // (index a + 65) must go to the smaller index although the lane order is the other way round
          if (a + 1 + 63 < n_d && a + 1 + 63 != a) {
            std::vector<double> d2 = det;
            const int lo = a + 1, hi = a + 64;  // lanes (a + 1) % 64 and a % 64
            d2[2 * hi] = d2[2 * lo];
            d2[2 * hi + 1] = d2[2 * lo + 1];
            pt[0] = d2[2 * lo] - 1.0;
            pt[1] = d2[2 * lo + 1] + 2.0;
            check_set(pt, n_m, d2, n_d, 5.0, "tie across lanes");
            ++g_ties;
          }
        }
        // predictions exactly nn_tol away (3-4-5 offsets on integer coordinates: d2 = 25 exactly): `<=` keeps them,
        // the next smaller tolerance does not
        if (n_d >= 1) {
          std::vector<double> di((size_t)2 * n_d), pe((size_t)2 * n_m);
          for (int j = 0; j < n_d; ++j) {
            di[2 * j] = 20.0 * (j % 32) + 10.0;
            di[2 * j + 1] = 20.0 * (j / 32) + 10.0;
          }
          for (int i = 0; i < n_m; ++i) {
            const int j = (int)(rng() % (unsigned)n_d);
            pe[2 * i] = di[2 * j] + ((i & 1) ? 3.0 : -4.0);
            pe[2 * i + 1] = di[2 * j + 1] + ((i & 1) ? -4.0 : 3.0);
          }
          unsigned cm[MPE_MAX_MARKERS], cd[MPE_MAX_MARKERS];
          const int kept = plain_rows(pe.data(), n_m, di.data(), n_d, 5.0, cm, cd);
          CHECK(kept == n_m, "edge: %d of %d predictions at exactly nn_tol kept", kept, n_m);
          g_edge_kept += kept;
          check_set(pe, n_m, di, n_d, 5.0, "edge kept");
          const double below = std::nextafter(5.0, 0.0);
          CHECK(plain_rows(pe.data(), n_m, di.data(), n_d, below, cm, cd) == 0, "edge: rows kept below nn_tol");
          check_set(pe, n_m, di, n_d, below, "edge dropped");
        }
        // NaN predictions (detection only: no rows), one NaN prediction among good ones, NaN detections (never win)
        {
          std::vector<double> pn((size_t)2 * n_m, nan);
          check_set(pn, n_m, det, n_d, 5.0, "nan predictions");
          unsigned cm[MPE_MAX_MARKERS], cd[MPE_MAX_MARKERS];
          CHECK(lane_rows(pn.data(), n_m, det.data(), n_d, 5.0, cm, cd) == 0, "nan predictions made rows");
          std::vector<double> p1 = pred;
          p1[2 * (n_m / 2)] = nan;
          check_set(p1, n_m, det, n_d, 5.0, "one nan prediction");
          std::vector<double> dn = det;
          for (int j = 0; j < n_d; j += 3) dn[2 * j + (j & 1)] = nan;
          check_set(pred, n_m, dn, n_d, 5.0, "nan detections");
          std::vector<double> da((size_t)2 * (n_d > 0 ? n_d : 1), nan);
          check_set(pred, n_m, da, n_d, std::numeric_limits<double>::infinity(), "all nan, infinite tolerance");
        }
      }
  // detection index 256 survives the hand-over
  {
    std::vector<double> det(512), pred(8);
    for (int j = 0; j < 256; ++j) {
      det[2 * j] = 3.0 * j;
      det[2 * j + 1] = 100.0;
    }
    for (int i = 0; i < 4; ++i) {
      pred[2 * i] = det[2 * (255 - i)] + 0.5;
      pred[2 * i + 1] = 100.5;
    }
    unsigned cm[MPE_MAX_MARKERS], cd[MPE_MAX_MARKERS];
    const int nc = lane_rows(pred.data(), 4, det.data(), 256, 5.0, cm, cd);
    CHECK(nc == 4 && cd[0] == 256 && cd[3] == 253, "index 256: %d rows, first names %u", nc, nc ? cd[0] : 0);
    check_set(pred, 4, det, 256, 5.0, "index 256");
  }
  CHECK(g_shared > 100, "only %lld rows shared a detection", g_shared);
  if (g_failed) {
    std::printf("wide_nn_host: %d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("wide_nn_host ok: %lld sets, %lld rows, %lld ties, %lld shared, %lld kept at the tolerance\n", g_sets, g_rows, g_ties,
              g_shared, g_edge_kept);
  return 0;
}
