// mpe_brute_blocks.h — the block table of k2_vote_setups (mpe_k2.hip): which block of the one voting launch of
// mpe_solve_bruteforce_batch_setups works on which share of which item.  Plain C++ in a header of its own so that the
// CPU tier compiles it for the host (tests/host/brute_blocks_host.cpp) and runs it under AddressSanitizer.
//
// An item (one detection set with its set-up's markers) has C(n_det, 3) * P(n_markers, 3) hypotheses — 96 at 4 / 4,
// 600 at 5 / 5, 73 920 at 12 / 8, 2.5 M at 64 / 5, 140 M at 64 / 16.  Block `part` of `parts` of an item takes the
// hypotheses t = part * threads + tid, stepping parts * threads (k2_strict_frame): every hypothesis belongs to exactly
// one (block, stride) pair whatever `parts` is, and integer votes do not depend on who casts them.  parts grows with
// the hypothesis count — one block per kBruteHypPerBlock hypotheses — up to `cap` blocks per item, so that one wide
// item spreads over the chip while 64 five-detection items stay 64 blocks.  The share of an item depends on that item
// and the cap alone: its entries are the same whatever else is in the list.  An item that cannot vote (fewer than 4
// detections or markers: initialise() needs an unused detection and an unused marker) gets no block.
#pragma once
#include <stdint.h>

#include <vector>

namespace mpe {

struct BruteBlock {  // (device table, one entry per block of the launch)
  int item;   // the caller's item index
  int part;   // this block's share ...
  int parts;  // ... of so many of that item
  int pad_;
};
static_assert(sizeof(BruteBlock) == 16, "table entries of 16 bytes");

// hypotheses per block: four rounds of a 256-thread block.  (A strict hypothesis is a chain of dependent FP64
// operations of tens of microseconds per lane; fewer rounds per block shorten an item's latency, more blocks than the
// chip holds at once do not.)
constexpr long long kBruteHypPerBlock = 1024;

inline long long brute_hypotheses(int n_det, int n_markers) {
  if (n_det < 4 || n_markers < 4) return 0;
  const long long combos = (long long)n_det * (n_det - 1) * (n_det - 2) / 6;
  return combos * n_markers * (n_markers - 1) * (n_markers - 2);
}

// blocks of an item of `hyp` hypotheses, at most cap (cap < 1 counts as 1)
inline int brute_parts(long long hyp, int cap) {
  if (hyp <= 0) return 0;
  const long long want = (hyp + kBruteHypPerBlock - 1) / kBruteHypPerBlock;
  const long long lim = cap < 1 ? 1 : cap;
  return (int)(want < lim ? want : lim);
}

// The table of n items in item order, an item's parts in ascending order; n_markers[i] is the marker count of item i's
// set-up.  Returns the number of blocks.
inline size_t brute_block_table(const int* n_det, const int* n_markers, int n, int cap, std::vector<BruteBlock>& tab) {
  tab.clear();
  for (int i = 0; i < n; ++i) {
    const int parts = brute_parts(brute_hypotheses(n_det[i], n_markers[i]), cap);
    for (int p = 0; p < parts; ++p) tab.push_back(BruteBlock{i, p, parts, 0});
  }
  return tab.size();
}

}  // namespace mpe
