// wide_peel_host.cpp — the peel-and-compact logic of k3_peel_wide (csrc/mpe_wide_peel.h) as a stand-alone host program,
// against the oracle's correspondencesFromHistogram (oracle/mpe_oracle.cpp, linked in): a few thousand random integer
// histograms of 4 .. 256 detections x 4 .. 16 markers with ties, duplicate rows, all-zero columns and all-zero tables,
// under several thresholds; the re-indexing into the compact record must round-trip; and the block table of
// csrc/mpe_brute_blocks.h for sets of up to 256 detections / 16 markers must hand every hypothesis to exactly one
// (block, lane, stride) triple for both block sizes the wide voting launch uses.  Built plain and with
// -fsanitize=address,undefined (tools/host_sanitize.sh); prints "wide_peel_host ok: ..." and returns 0, or says what
// failed and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mpe_brute_blocks.h"
#include "mpe_wide_peel.h"
#include "../../oracle/mpe_oracle.h"

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

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}
int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

// what k3_peel_wide does for one item, on the host: column maxima (one per lane there), peel, compact
struct Peeled {
  int n_c = 0, n_s = 0;
  unsigned cm[MPE_MAX_MARKERS], cd[MPE_MAX_MARKERS], slot_wide[MPE_MAX_MARKERS], cslot[MPE_MAX_MARKERS];
};
Peeled peel(const std::vector<uint32_t>& H16, int n_det, int n_m, unsigned thr) {
  Peeled p;
  unsigned colmax[MPE_MAX_MARKERS], colrow[MPE_MAX_MARKERS];
  for (int c = 0; c < n_m; ++c) mpe::wide_column_max(H16.data(), n_det, c, colmax[c], colrow[c]);
  p.n_c = mpe::wide_peel_rows(colmax, colrow, n_m, thr, p.cm, p.cd);
  p.n_s = mpe::wide_compact_rows(p.cd, p.n_c, p.slot_wide, p.cslot);
  return p;
}

void check_case(const std::vector<uint32_t>& dense, int n_det, int n_m, unsigned thr, const char* what, long& rows_seen,
                long& shared_seen) {
  std::vector<uint32_t> H16((size_t)n_det * MPE_MAX_MARKERS, 0xDEADu);  // (columns beyond n_m must never be read)
  bool all_zero = true;
  for (int r = 0; r < n_det; ++r)
    for (int c = 0; c < n_m; ++c) {
      H16[(size_t)r * MPE_MAX_MARKERS + c] = dense[(size_t)r * n_m + c];
      all_zero &= dense[(size_t)r * n_m + c] == 0;
    }
  const Peeled p = peel(H16, n_det, n_m, thr);
  std::vector<uint32_t> consumed(dense), ref((size_t)2 * n_m, 0);
  int n_ref = orc_correspondences_from_histogram(consumed.data(), n_det, n_m, thr, ref.data());
  if (all_zero) n_ref = 0;  // initialise() returns before correspondencesFromHistogram (pose_estimator.cpp:704)
  CHECK(p.n_c == n_ref, "%s %d x %d thr %u: %d rows, oracle %d", what, n_det, n_m, thr, p.n_c, n_ref);
  if (p.n_c != n_ref) return;
  for (int i = 0; i < p.n_c; ++i) {
    CHECK(p.cm[i] == ref[(size_t)2 * i] && p.cd[i] == ref[(size_t)2 * i + 1], "%s %d x %d thr %u row %d: (%u, %u), oracle (%u, %u)",
          what, n_det, n_m, thr, i, p.cm[i], p.cd[i], ref[(size_t)2 * i], ref[(size_t)2 * i + 1]);
    CHECK(p.cd[i] >= 1 && p.cd[i] <= (unsigned)n_det, "detection index %u of %d", p.cd[i], n_det);
  }
  // the re-indexing round-trips: distinct detections, distinct slots in ascending wide index; shared detection, shared slot
  int distinct = 0;
  for (int i = 0; i < p.n_c; ++i) {
    bool seen = false;
    for (int j = 0; j < i; ++j) seen |= p.cd[j] == p.cd[i];
    distinct += seen ? 0 : 1;
  }
  CHECK(p.n_s == distinct && p.n_s <= p.n_c, "%d slots for %d distinct detections", p.n_s, distinct);
  for (int k = 0; k < MPE_MAX_MARKERS; ++k) {
    if (k < p.n_s) CHECK(p.slot_wide[k] >= 1 && (k == 0 || p.slot_wide[k] > p.slot_wide[k - 1]), "slot %d not ascending", k);
    else CHECK(p.slot_wide[k] == 0, "slot %d beyond the %d slots holds %u", k, p.n_s, p.slot_wide[k]);
  }
  for (int i = 0; i < p.n_c; ++i) {
    CHECK(p.cslot[i] >= 1 && p.cslot[i] <= (unsigned)p.n_s, "row %d: slot %u of %d", i, p.cslot[i], p.n_s);
    if (p.cslot[i] >= 1 && p.cslot[i] <= (unsigned)p.n_s)
      CHECK(p.slot_wide[p.cslot[i] - 1] == p.cd[i], "row %d: slot %u maps back to %u, not %u", i, p.cslot[i],
            p.slot_wide[p.cslot[i] - 1], p.cd[i]);
  }
  rows_seen += p.n_c;
  shared_seen += p.n_c - p.n_s;
}

// hypotheses that the blocks of `tab` walk for an item of `hyp` hypotheses with `threads` lanes, by counting
long long walked(const std::vector<mpe::BruteBlock>& tab, int item, long long hyp, int threads) {
  long long n = 0;
  for (const mpe::BruteBlock& b : tab) {
    if (b.item != item) continue;
    const long long stride = (long long)b.parts * threads;
    for (int tid = 0; tid < threads; ++tid) {
      const long long first = (long long)b.part * threads + tid;
      if (first < hyp) n += (hyp - first + stride - 1) / stride;
    }
  }
  return n;
}
}  // namespace

int main() {
  long cases = 0, rows_seen = 0, shared_seen = 0;
  for (int it = 0; it < 4000; ++it) {
    const int n_det = (it % 7 == 0) ? 256 : rnd_in(4, 256), n_m = rnd_in(4, 16);
    const int kind = it % 8;
    std::vector<uint32_t> H((size_t)n_det * n_m, 0);
    const uint32_t top = kind < 3 ? 3u : (kind < 6 ? 40u : 100000u);  // (small ranges: ties everywhere)
    const int fill_pct = kind == 7 ? 2 : rnd_in(5, 100);
    for (auto& v : H) v = (rnd() % 100 < (uint32_t)fill_pct) ? rnd() % (top + 1) : 0u;
    if (kind == 1 || kind == 4)  // all-zero columns
      for (int c = 0; c < n_m; ++c)
        if (rnd() % 3 == 0)
          for (int r = 0; r < n_det; ++r) H[(size_t)r * n_m + c] = 0;
    if (kind == 2 || kind == 5)  // duplicate rows (the same maximum in several rows of a column: the first one wins)
      for (int k = 0; k < 8; ++k) {
        const int a = rnd_in(0, n_det - 1), b = rnd_in(0, n_det - 1);
        std::memcpy(&H[(size_t)a * n_m], &H[(size_t)b * n_m], sizeof(uint32_t) * n_m);
      }
    if (kind == 3)  // one detection wins several columns: named by several markers
      for (int c = 0; c < n_m; c += 2) H[(size_t)(n_det - 1) * n_m + c] = top + 1 + (uint32_t)c;
    if (it % 50 == 49) std::fill(H.begin(), H.end(), 0u);  // all-zero table
    const unsigned n3 = (unsigned)(n_m * (n_m - 1) * (n_m - 2) / 6);
    const unsigned thrs[4] = {n3, 0u, 1u, (unsigned)rnd_in(0, (int)top + 2)};
    for (unsigned thr : thrs) {
      check_case(H, n_det, n_m, thr, "random", rows_seen, shared_seen);
      ++cases;
    }
  }
  {  // the last detection of a full set wins: its 1-based index 256 does not fit a byte
    const int n_det = MPE_WIDE_DETECTIONS, n_m = 5;
    std::vector<uint32_t> H((size_t)n_det * n_m, 1);
    H[(size_t)255 * n_m + 2] = 90;
    H[(size_t)254 * n_m + 0] = 80;
    H[(size_t)255 * n_m + 4] = 70;
    check_case(H, n_det, n_m, 10, "last", rows_seen, shared_seen);
    std::vector<uint32_t> H16((size_t)n_det * MPE_MAX_MARKERS, 0);
    for (int r = 0; r < n_det; ++r)
      for (int c = 0; c < n_m; ++c) H16[(size_t)r * MPE_MAX_MARKERS + c] = H[(size_t)r * n_m + c];
    const Peeled p = peel(H16, n_det, n_m, 10);
    CHECK(p.n_c == 3 && p.cd[0] == 256 && p.cd[1] == 255 && p.cd[2] == 256, "rows %d: %u %u %u", p.n_c, p.cd[0], p.cd[1], p.cd[2]);
    CHECK(p.n_s == 2 && p.slot_wide[0] == 255 && p.slot_wide[1] == 256, "slots %d: %u %u", p.n_s, p.slot_wide[0], p.slot_wide[1]);
    CHECK(p.cslot[0] == 2 && p.cslot[1] == 1 && p.cslot[2] == 2, "compact rows %u %u %u", p.cslot[0], p.cslot[1], p.cslot[2]);
    ++cases;
  }
  // the block table for wide sets: counts, and every hypothesis walked once whatever the block size
  CHECK(mpe::brute_hypotheses(256, 16) == 2763520LL * 3360LL, "%lld", mpe::brute_hypotheses(256, 16));
  CHECK(mpe::brute_hypotheses(256, 4) == 2763520LL * 24LL, "%lld", mpe::brute_hypotheses(256, 4));
  CHECK(mpe::brute_hypotheses(65, 4) == 43680LL * 24LL, "%lld", mpe::brute_hypotheses(65, 4));
  {
    const int nd[6] = {256, 65, 3, 129, 256, 100}, nm[6] = {16, 16, 16, 16, 16, 16};
    const int caps[3] = {1, 1024, 100000};
    for (int cap : caps) {
      std::vector<mpe::BruteBlock> tab;
      const size_t nb = mpe::brute_block_table(nd, nm, 6, cap, tab);
      CHECK(nb == tab.size() && nb <= (size_t)5 * (size_t)cap, "%zu blocks under cap %d", nb, cap);
      for (int i = 0; i < 6; ++i) {
        const long long hyp = mpe::brute_hypotheses(nd[i], nm[i]);
        CHECK(walked(tab, i, hyp, 256) == hyp, "item %d cap %d, 256 lanes: %lld of %lld", i, cap, walked(tab, i, hyp, 256), hyp);
        CHECK(walked(tab, i, hyp, 128) == hyp, "item %d cap %d, 128 lanes: %lld of %lld", i, cap, walked(tab, i, hyp, 128), hyp);
      }
    }
  }
  if (g_failed) {
    std::printf("wide_peel_host: %d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("wide_peel_host ok: %ld histograms, %ld rows, %ld shared detections\n", cases, rows_seen, shared_seen);
  return 0;
}
