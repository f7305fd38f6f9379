// brute_blocks_host.cpp — the block table of k2_vote_setups (csrc/mpe_brute_blocks.h) as a stand-alone host program:
// the shares the table hands out are walked exactly as k2_strict_frame walks them (t = part * threads + tid, stepping
// parts * threads) and every hypothesis of every item must be met exactly once.  Built plain and with
// -fsanitize=address,undefined (tools/host_sanitize.sh); prints "brute_blocks_host ok: ..." and returns 0, or says what
// failed and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mpe_brute_blocks.h"

using mpe::BruteBlock;

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

struct Item {
  int n_det, n_markers;
  long long hyp;  // expected hypothesis count
};

// every hypothesis of every item exactly once; no block for an item that cannot vote; parts consistent and ascending
long long check_table(const std::vector<Item>& items, int cap, int threads, const std::vector<BruteBlock>& tab) {
  long long walked = 0;
  std::vector<std::vector<unsigned char> > seen(items.size());
  std::vector<int> next_part(items.size(), 0), parts_of(items.size(), 0);
  for (size_t i = 0; i < items.size(); ++i) seen[i].assign((size_t)items[i].hyp, 0);
  int last_item = -1;
  for (const BruteBlock& b : tab) {
    CHECK(b.item >= 0 && b.item < (int)items.size(), "item %d", b.item);
    if (b.item < 0 || b.item >= (int)items.size()) return walked;
    const Item& it = items[(size_t)b.item];
    CHECK(it.n_det >= 4 && it.n_markers >= 4, "block for item %d of %d detections, %d markers", b.item, it.n_det, it.n_markers);
    CHECK(b.item >= last_item, "items out of order at item %d", b.item);
    last_item = b.item;
    CHECK(b.parts >= 1 && b.parts <= (cap < 1 ? 1 : cap), "item %d: %d parts, cap %d", b.item, b.parts, cap);
    CHECK(b.part == next_part[(size_t)b.item], "item %d: part %d where %d was due", b.item, b.part, next_part[(size_t)b.item]);
    ++next_part[(size_t)b.item];
    if (parts_of[(size_t)b.item] == 0) parts_of[(size_t)b.item] = b.parts;
    CHECK(parts_of[(size_t)b.item] == b.parts, "item %d: parts %d and %d", b.item, parts_of[(size_t)b.item], b.parts);
    for (int tid = 0; tid < threads; ++tid)
      for (long long t = (long long)b.part * threads + tid; t < it.hyp; t += (long long)b.parts * threads) {
        ++seen[(size_t)b.item][(size_t)t];
        ++walked;
      }
  }
  for (size_t i = 0; i < items.size(); ++i) {
    CHECK(next_part[i] == parts_of[i], "item %zu: %d of %d parts listed", i, next_part[i], parts_of[i]);
    CHECK((items[i].hyp == 0) == (parts_of[i] == 0), "item %zu: %lld hypotheses, %d parts", i, items[i].hyp, parts_of[i]);
    long long bad = 0;
    for (unsigned char c : seen[i]) bad += c != 1;
    CHECK(bad == 0, "item %zu: %lld of %lld hypotheses not met exactly once", i, bad, items[i].hyp);
  }
  return walked;
}

size_t build(const std::vector<Item>& items, int cap, std::vector<BruteBlock>& tab) {
  std::vector<int> nd, nm;
  for (const Item& it : items) {
    nd.push_back(it.n_det);
    nm.push_back(it.n_markers);
  }
  return mpe::brute_block_table(nd.data(), nm.data(), (int)items.size(), cap, tab);
}
}  // namespace

int main() {
  const Item none3 = {3, 5, 0}, none0 = {0, 4, 0}, few_markers = {5, 3, 0}, h96 = {4, 4, 96}, h600 = {5, 5, 600},
             h73920 = {12, 8, 73920}, wide = {64, 5, 2499840};
  for (const Item& it : {none3, none0, few_markers, h96, h600, h73920, wide})
    CHECK(mpe::brute_hypotheses(it.n_det, it.n_markers) == it.hyp, "%d / %d: %lld", it.n_det, it.n_markers,
          mpe::brute_hypotheses(it.n_det, it.n_markers));
  CHECK(mpe::brute_hypotheses(64, 16) == 41664LL * 3360, "64 / 16");
  const std::vector<Item> mixed = {h600, none3, wide, h96, h73920, none0, h600, wide, few_markers, h73920, h96};
  long long walked = 0;
  int lists = 0;
  std::vector<BruteBlock> tab, one;
  // caps that bind (the wide items want 2442 blocks, the 73 920-hypothesis items 73) and one that does not
  for (int cap : {1, 7, 64, 1024, 4096})
    for (int threads : {256, 128}) {
      const size_t nb = build(mixed, cap, tab);
      CHECK(nb == tab.size(), "%zu blocks returned, %zu listed", nb, tab.size());
      walked += check_table(mixed, cap, threads, tab);
      ++lists;
      if (cap <= 1024) {
        size_t wide_blocks = 0;
        for (const BruteBlock& b : tab) wide_blocks += b.item == 2;
        CHECK(wide_blocks == (size_t)cap, "cap %d does not bind: %zu blocks for the wide item", cap, wide_blocks);
      }
      // a list of one item: that item's entries of the mixed list
      for (size_t i = 0; i < mixed.size(); ++i) {
        build({mixed[i]}, cap, one);
        size_t k = 0;
        for (const BruteBlock& b : tab) {
          if (b.item != (int)i) continue;
          CHECK(k < one.size() && one[k].item == 0 && one[k].part == b.part && one[k].parts == b.parts,
                "cap %d item %zu entry %zu differs from the single-item list", cap, i, k);
          ++k;
        }
        CHECK(k == one.size(), "cap %d item %zu: %zu entries, alone %zu", cap, i, k, one.size());
      }
    }
  // 64 five-detection items stay 64 blocks; one wide item spreads over the cap; small items are one block each
  const size_t nb64 = build(std::vector<Item>(64, h600), 1024, tab);
  CHECK(nb64 == 64, "%zu blocks for 64 five-detection items", nb64);
  walked += check_table(std::vector<Item>(64, h600), 1024, 256, tab);
  CHECK(build({wide}, 1024, tab) == 1024, "one wide item");
  CHECK(build({h96}, 1024, tab) == 1 && build({h73920}, 1024, tab) == 73, "small items");
  CHECK(build({}, 1024, tab) == 0 && build({none3, none0, few_markers}, 1024, tab) == 0, "lists without a voting item");
  if (g_failed) {
    std::printf("brute_blocks_host: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("brute_blocks_host ok: %d lists, %lld hypotheses walked\n", lists + 1, walked);
  return 0;
}
