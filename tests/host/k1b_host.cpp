// Host build of the DEVICE blob-extraction source (test scaffolding, CPU tier).
//
// tests/test_k1b_host.py cuts the region `struct BlobRec { ... }` .. `// final stage: kept blobs` out of
// rpg_monocular_pose_estimator_amd/csrc/mpe_k1.hip + mpe_kernels_common.h (threshold helpers, fixed-point blur, Suzuki border
// following, polygon sums, shape filter, undistortion — everything of K1b that is not wave plumbing) and
// `struct DetectParams` out of mpe_internal.h into k1b_extract.inc, and compiles this file with g++.  The shims
// below give the HIP spellings a one-lane meaning.  The flow of host_find_leds is that of the device's
// whole-frame tier (k1b_general): threshold -> blurred-mask bitmap -> raster scan with border following ->
// kept blobs in descending raster order of their start pixel -> undistortion.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using std::max;
using std::min;
#define __device__
#define __forceinline__ inline
#define __noinline__
#define __restrict__
#define MPE_MAX_KSIZE 9
typedef unsigned long long u64;
struct uint4 {
  unsigned x, y, z, w;
};
static inline uint4 make_uint4(unsigned x, unsigned y, unsigned z, unsigned w) { return uint4{x, y, z, w}; }
static inline void atomicOr(u64* p, u64 v) { *p |= v; }
static inline void atomicOr(unsigned* p, unsigned v) { *p |= v; }
static inline int __mul24(int a, int b) { return a * b; }
static inline u64 __builtin_amdgcn_ballot_w64(bool b) { return b ? 1 : 0; }
static inline unsigned __builtin_bitreverse32(unsigned v) {
  unsigned r = 0;
  for (int i = 0; i < 32; ++i)
    if ((v >> i) & 1) r |= 1u << (31 - i);
  return r;
}
static inline unsigned __builtin_amdgcn_alignbyte(unsigned hi, unsigned lo, unsigned sh) {
  return (unsigned)(((((u64)hi) << 32) | lo) >> (8 * (sh & 3)));
}
static inline unsigned __builtin_amdgcn_udot4(unsigned a, unsigned b, unsigned c, bool) {
  for (int i = 0; i < 4; ++i) c += ((a >> (8 * i)) & 0xFFu) * ((b >> (8 * i)) & 0xFFu);
  return c;
}
static inline int atomicAdd(int* p, int v) { const int o = *p; *p += v; return o; }
static inline int atomicMin(int* p, int v) { const int o = *p; if (v < o) *p = v; return o; }
static inline int atomicMax(int* p, int v) { const int o = *p; if (v > o) *p = v; return o; }
static inline void wave_sync() {}
// raw contour sums of both contour phases (scan_window: the border trace; cells_phase: cell sums), see host_cells_vs_trace
struct RawRec {
  long long a00, a10, a01;
  int xmin, xmax, ymin, ymax;
  unsigned key;
};
static std::vector<RawRec>* g_raw = nullptr;
#define K1B_ON_BLOBREC(rec, key) \
  do { if (g_raw) g_raw->push_back(RawRec{(rec).a00, (rec).a10, (rec).a01, (rec).xmin, (rec).xmax, (rec).ymin, (rec).ymax, (key)}); } while (0)
#define K1B_CELL_LANE_ITEMS 192  // (one "lane" owns every item of the frame here)
#define __host__
#include "k1a_extract.inc"  // ThrTest, make_thr_test, gt_word, maybe_gt16, any_gt16 (`struct ThrTest {` .. `#ifndef K1A_UNROLL`)
#include "k1b_extract.inc"

extern "C" int host_find_leds(const uint8_t* img, int rows, int cols, int thr, const int* taps, int ksize,
                              const double* shape /* min_area max_area max_wh max_circ */, const double* K,
                              const double* D, int nD, int roi_x, int roi_y, float* dist_xy, double* undist_xy,
                              int cap) {
  DetectParams dp;
  std::memset(&dp, 0, sizeof(dp));
  dp.thr = thr;
  dp.ksize = ksize;
  for (int i = 0; i < ksize; ++i) dp.taps[i] = taps[i];
  pack_taps(dp);
  dp.min_area = shape[0];
  dp.max_area = shape[1];
  dp.max_wh = shape[2];
  dp.max_circ = shape[3];
  for (int i = 0; i < 9; ++i) dp.K[i] = K[i];
  dp.ifx = 1. / K[0];
  dp.ify = 1. / K[4];
  for (int i = 0; i < 8; ++i) dp.k[i] = i < nD ? D[i] : 0.0;
  dp.undist_iters = nD > 0 ? 5 : 0;
  dp.roi_x = roi_x;
  dp.roi_y = roi_y;
  // thresholded pixels, rows of 16-byte segments (THRESH_TOZERO four bytes at a time as the device does)
  const int nseg = (cols + 15) / 16, PW = 16 * nseg;
  std::vector<uint8_t> pix((size_t)rows * PW, 0);
  for (int y = 0; y < rows; ++y) std::memcpy(&pix[(size_t)y * PW], img + (size_t)y * cols, cols);
  const unsigned add = (unsigned)(255 - thr) * 0x00010001u;
  for (size_t i = 0; i < pix.size(); i += 4) {
    unsigned w;
    std::memcpy(&w, &pix[i], 4);
    w = tozero4(w, add);
    std::memcpy(&pix[i], &w, 4);
  }
  const int wb = (cols + 2 + 63) / 64;
  std::vector<u64> nz((size_t)(rows + 2) * wb + 1, 0), pm(nz.size(), 0), ng(nz.size(), 0);
  const PixWin pw = {pix.data(), 0, rows, 0, PW, 0u, nullptr, 0};
  for (int y = 0; y < rows; ++y)
    for (int c = 0; c < nseg; ++c) blur_to_bitmap(pw, rows, cols, dp, dp.taps, y, c, nz.data() + (size_t)(y + 1) * wb, 0);
  struct Kept {
    float x, y;
    unsigned key;
  };
  std::vector<Kept> kept;
  int over = 0;
  scan_window(nz.data(), pm.data(), ng.data(), wb, rows, 0, 0, dp, roi_x, roi_y, &over,
              [&](float mcx, float mcy, unsigned key) { kept.push_back({mcx, mcy, key}); });
  if (over) return -1;
  std::sort(kept.begin(), kept.end(), [](const Kept& a, const Kept& b) { return a.key > b.key; });
  const int n = (int)kept.size();
  for (int i = 0; i < n && i < cap; ++i) {
    float ux, uy;
    undistort_point(kept[i].x, kept[i].y, dp, ux, uy);
    dist_xy[2 * i] = kept[i].x;
    dist_xy[2 * i + 1] = kept[i].y;
    undist_xy[2 * i] = (double)ux;
    undist_xy[2 * i + 1] = (double)uy;
  }
  return n;
}

// lds_set_range — how the front phase marks the rows within +-r of a bright segment in its row bitset (s_rowact, 64 words:
// a bit per row of a frame of up to 4 096 rows) — over n inclusive ranges lohi[2 i] .. lohi[2 i + 1], each shorter than 64.
extern "C" void host_set_row_ranges(u64* bits, const int* lohi, int n) {
  for (int i = 0; i < n; ++i) lds_set_range(bits, lohi[2 * i], lohi[2 * i + 1]);
}

// The image scan's per-segment tests (k1a_scan and the voting kernel's scan rider): bit 0 = any_gt16, bit 1 = maybe_gt16
extern "C" int host_scan_tests(const uint8_t* seg16, int thr) {
  uint4 v;
  std::memcpy(&v, seg16, 16);
  const ThrTest q = make_thr_test(thr);
  // bits 2 / 3: the same through the compile-time forms the kernels branch to (k1a_scan, the rider's first level)
  const unsigned a_c = q.sel ? any_gt16_c<true>(v, q.kk) : any_gt16_c<false>(v, q.kk);
  const unsigned m_c = q.sel ? maybe_gt16_c<true>(v, q.kk) : maybe_gt16_c<false>(v, q.kk);
  return (any_gt16(v, q) ? 1 : 0) | (maybe_gt16(v, q) ? 2 : 0) | (a_c ? 4 : 0) | (m_c ? 8 : 0);
}


// The contour phase without border following (cells_phase) against the border trace (scan_window) on a binary mask cut
// into island windows {y0, y1, x0, x1} (half-open; the caller keeps the windows' contents independent): the raw contour
// sums (orientation-normalised), bounding boxes and start keys of every component must agree, and so must the blobs
// that pass the shape filter.  Returns the number of components compared (>= 0), -1 on a mismatch; *n_fallback = islands
// the cell phase handed back to the trace (holes, capacity).
extern "C" int host_cells_vs_trace(const uint8_t* mask, int rows, int cols, const int* wins, int n_win,
                                   const double* shape, int* n_fallback) {
  DetectParams dp;
  std::memset(&dp, 0, sizeof(dp));
  dp.min_area = shape[0];
  dp.max_area = shape[1];
  dp.max_wh = shape[2];
  dp.max_circ = shape[3];
  std::vector<CellIsl> cs(n_win);
  int off = 0;
  for (int k = 0; k < n_win; ++k) {
    const int y0 = wins[4 * k], y1 = wins[4 * k + 1], x0 = wins[4 * k + 2], x1 = wins[4 * k + 3];
    cs[k].bm_off = off;
    cs[k].W = ((x1 - x0) + 2 + 63) / 64;
    cs[k].H = y1 - y0;
    cs[k].ylo = y0;
    cs[k].xw0 = x0;
    off += (cs[k].H + 2) * cs[k].W;
  }
  std::vector<u64> nz((size_t)off + 2, 0), pm(nz.size(), 0), ng(nz.size(), 0);
  for (int k = 0; k < n_win; ++k)
    for (int y = 0; y < cs[k].H; ++y)
      for (int x = cs[k].xw0; x < wins[4 * k + 3]; ++x)
        if (mask[(size_t)(cs[k].ylo + y) * cols + x]) {
          const int xb = x - cs[k].xw0 + 1;
          nz[cs[k].bm_off + (size_t)(y + 1) * cs[k].W + (xb >> 6)] |= 1ull << (xb & 63);
        }
  struct Kept {
    float x, y;
    unsigned key;
    bool operator<(const Kept& o) const { return key < o.key; }
    bool operator==(const Kept& o) const { return key == o.key && std::memcmp(&x, &o.x, 4) == 0 && std::memcmp(&y, &o.y, 4) == 0; }
  };
  std::vector<Kept> kt, kc;
  std::vector<RawRec> rt, rc;
  int over = 0;
  g_raw = &rt;
  for (int k = 0; k < n_win; ++k)
    scan_window(nz.data() + cs[k].bm_off, pm.data() + cs[k].bm_off, ng.data() + cs[k].bm_off, cs[k].W, cs[k].H,
                cs[k].ylo, cs[k].xw0, dp, 0, 0, &over, [&](float mx, float my, unsigned key) { kt.push_back({mx, my, key}); });
  std::fill(pm.begin(), pm.end(), 0);
  std::fill(ng.begin(), ng.end(), 0);
  g_raw = &rc;
  const unsigned todo = cells_phase(nz.data(), pm.data(), ng.data(), cs.data(), n_win, 0, 1, dp, 0, 0,
                                    [&](float mx, float my, unsigned key) { kc.push_back({mx, my, key}); });
  // islands handed back: the product then runs scan_window on them (mark bitmaps must be clean again)
  *n_fallback = 0;
  for (int k = 0; k < n_win; ++k) {
    if (!((todo >> k) & 1u)) continue;
    ++*n_fallback;
    for (int i = 0; i < (cs[k].H + 2) * cs[k].W; ++i)
      if (pm[cs[k].bm_off + i] || ng[cs[k].bm_off + i]) {
        g_raw = nullptr;
        return -1;
      }
    // drop what the cell phase recorded for this island before giving up, then let the trace speak
    const unsigned klo = (unsigned)cs[k].ylo << 12, khi = (unsigned)(cs[k].ylo + cs[k].H) << 12;
    auto in_island = [&](unsigned key) {
      const int x = (int)(key & 0xFFF);
      return key >= klo && key < khi && x >= cs[k].xw0 && x < wins[4 * k + 3];
    };
    rc.erase(std::remove_if(rc.begin(), rc.end(), [&](const RawRec& r) { return in_island(r.key); }), rc.end());
    scan_window(nz.data() + cs[k].bm_off, pm.data() + cs[k].bm_off, ng.data() + cs[k].bm_off, cs[k].W, cs[k].H,
                cs[k].ylo, cs[k].xw0, dp, 0, 0, &over, [&](float mx, float my, unsigned key) { kc.push_back({mx, my, key}); });
  }
  g_raw = nullptr;
  if (over) return -1;
  auto norm = [](std::vector<RawRec>& v) {
    for (auto& r : v)
      if (r.a00 < 0) {
        r.a00 = -r.a00;
        r.a10 = -r.a10;
        r.a01 = -r.a01;
      }
    std::sort(v.begin(), v.end(), [](const RawRec& a, const RawRec& b) { return a.key < b.key; });
  };
  norm(rt);
  norm(rc);
  if (std::getenv("K1B_HOST_DEBUG")) {
    for (auto& r : rt) std::fprintf(stderr, "trace a00 %lld a10 %lld a01 %lld bbox %d %d %d %d key %u\n", r.a00, r.a10, r.a01, r.xmin, r.xmax, r.ymin, r.ymax, r.key);
    for (auto& r : rc) std::fprintf(stderr, "cells a00 %lld a10 %lld a01 %lld bbox %d %d %d %d key %u\n", r.a00, r.a10, r.a01, r.xmin, r.xmax, r.ymin, r.ymax, r.key);
  }
  if (rt.size() != rc.size()) return -1;
  for (size_t i = 0; i < rt.size(); ++i)
    if (rt[i].a00 != rc[i].a00 || rt[i].a10 != rc[i].a10 || rt[i].a01 != rc[i].a01 || rt[i].xmin != rc[i].xmin ||
        rt[i].xmax != rc[i].xmax || rt[i].ymin != rc[i].ymin || rt[i].ymax != rc[i].ymax || rt[i].key != rc[i].key)
      return -1;
  std::sort(kt.begin(), kt.end());
  std::sort(kc.begin(), kc.end());
  if (!(kt == kc)) return -1;
  return (int)rt.size();
}


// The general tier's decomposition (k1b_general, round 5): the whole-frame raster scan against ONE scan per BAND,
// called exactly as the kernel calls it (base pointers offset by lo * wb, H = its rows, ylo = lo, xw0 = 0).  A band is a
// maximal run of non-empty rows in which every row TOUCHES the one above it (some set pixel 8-adjacent to a set pixel
// of the previous row): no component crosses a boundary between two rows that do not touch, and a component below
// such a boundary cannot lie in a hole of one above it, so the raster scan decomposes there as it does at an empty
// row — which is what cuts uniformly spread noise (no empty rows at all) into a hundred bands.  The row above a band's
// first row may hold pixels now, but none of them is a neighbour of a pixel of the band, so no border following
// leaves the band.  Raw contour sums, bounding boxes, start keys and the blobs that pass the shape filter must agree.
// Returns the number of components (>= 0), -1 on a mismatch; *n_bands = bands found.
extern "C" int host_bands_vs_whole(const uint8_t* mask, int rows, int cols, const double* shape, int* n_bands) {
  DetectParams dp;
  std::memset(&dp, 0, sizeof(dp));
  dp.min_area = shape[0];
  dp.max_area = shape[1];
  dp.max_wh = shape[2];
  dp.max_circ = shape[3];
  const int wb = (cols + 2 + 63) / 64 + 1;  // (+ the pad word the pools end in)
  std::vector<u64> nz((size_t)(rows + 2) * wb + 1, 0), pm(nz.size(), 0), ng(nz.size(), 0);
  std::vector<int> active(rows, 0), linked(rows, 0);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x)
      if (mask[(size_t)y * cols + x]) {
        const int xb = x + 1;
        nz[(size_t)(y + 1) * wb + (xb >> 6)] |= 1ull << (xb & 63);
        active[y] = 1;
      }
  // linked[y]: row y touches row y - 1 — the device's word arithmetic (k1b_rows_touch) on the bitmap rows
  for (int y = 1; y < rows; ++y)
    linked[y] = k1b_rows_touch(nz.data() + (size_t)(y + 1) * wb, nz.data() + (size_t)y * wb, wb) ? 1 : 0;
  struct Kept {
    float x, y;
    unsigned key;
    bool operator<(const Kept& o) const { return key < o.key; }
    bool operator==(const Kept& o) const { return key == o.key && std::memcmp(&x, &o.x, 4) == 0 && std::memcmp(&y, &o.y, 4) == 0; }
  };
  std::vector<Kept> kw, kb;
  std::vector<RawRec> rw, rb;
  int over = 0;
  g_raw = &rw;
  scan_window(nz.data(), pm.data(), ng.data(), wb, rows, 0, 0, dp, 0, 0, &over,
              [&](float mx, float my, unsigned key) { kw.push_back({mx, my, key}); });
  std::fill(pm.begin(), pm.end(), 0);
  std::fill(ng.begin(), ng.end(), 0);
  g_raw = &rb;
  *n_bands = 0;
  for (int y = 0; y < rows;) {
    if (!active[y]) {
      ++y;
      continue;
    }
    int hi = y;
    while (hi + 1 < rows && active[hi + 1] && linked[hi + 1]) ++hi;
    // (the test's own check: a band window that starts one row late — the wrong base pointer — must be caught)
    const size_t off = (size_t)(y + (std::getenv("K1B_HOST_BREAK_BANDS") ? 1 : 0)) * wb;
    scan_window(nz.data() + off, pm.data() + off, ng.data() + off, wb, hi - y + 1, y, 0, dp, 0, 0, &over,
                [&](float mx, float my, unsigned key) { kb.push_back({mx, my, key}); });
    ++*n_bands;
    y = hi + 1;
  }
  g_raw = nullptr;
  if (over) return -1;
  auto norm = [](std::vector<RawRec>& v) {
    std::sort(v.begin(), v.end(), [](const RawRec& a, const RawRec& b) { return a.key < b.key; });
  };
  norm(rw);
  norm(rb);
  if (rw.size() != rb.size()) return -1;
  for (size_t i = 0; i < rw.size(); ++i)
    if (rw[i].a00 != rb[i].a00 || rw[i].a10 != rb[i].a10 || rw[i].a01 != rb[i].a01 || rw[i].xmin != rb[i].xmin ||
        rw[i].xmax != rb[i].xmax || rw[i].ymin != rb[i].ymin || rw[i].ymax != rb[i].ymax || rw[i].key != rb[i].key)
      return -1;
  std::sort(kw.begin(), kw.end());
  std::sort(kb.begin(), kb.end());
  if (!(kw == kb)) return -1;
  return (int)rw.size();
}


// Round 6: ... and every band cut again at its empty COLUMNS — the (band, column run) items of k1b_general: runs from
// window_column_runs, each scanned by scan_window<true> with its column range, called as the kernel calls them (all runs
// of a band share the band's rows and mark bitmaps).  Against the whole-frame scan: raw contour sums, boxes, keys, filtered
// blobs.  Returns the number of components (>= 0), -1 on a mismatch; *n_runs = items found.
extern "C" int host_runs_vs_whole(const uint8_t* mask, int rows, int cols, const double* shape, int* n_runs) {
  DetectParams dp;
  std::memset(&dp, 0, sizeof(dp));
  dp.min_area = shape[0];
  dp.max_area = shape[1];
  dp.max_wh = shape[2];
  dp.max_circ = shape[3];
  const int wb = (cols + 2 + 63) / 64 + 1;
  if (wb > 64) return -2;  // (the kernel's limit: 64 lanes hold a bitmap row's words)
  std::vector<u64> nz((size_t)(rows + 2) * wb + 1, 0), pm(nz.size(), 0), ng(nz.size(), 0);
  std::vector<int> active(rows, 0), linked(rows, 0);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x)
      if (mask[(size_t)y * cols + x]) {
        const int xb = x + 1;
        nz[(size_t)(y + 1) * wb + (xb >> 6)] |= 1ull << (xb & 63);
        active[y] = 1;
      }
  for (int y = 1; y < rows; ++y)
    linked[y] = k1b_rows_touch(nz.data() + (size_t)(y + 1) * wb, nz.data() + (size_t)y * wb, wb) ? 1 : 0;
  struct Kept {
    float x, y;
    unsigned key;
    bool operator<(const Kept& o) const { return key < o.key; }
    bool operator==(const Kept& o) const { return key == o.key && std::memcmp(&x, &o.x, 4) == 0 && std::memcmp(&y, &o.y, 4) == 0; }
  };
  std::vector<Kept> kw, kb;
  std::vector<RawRec> rw, rb;
  int over = 0;
  g_raw = &rw;
  scan_window(nz.data(), pm.data(), ng.data(), wb, rows, 0, 0, dp, 0, 0, &over,
              [&](float mx, float my, unsigned key) { kw.push_back({mx, my, key}); });
  std::fill(pm.begin(), pm.end(), 0);
  std::fill(ng.begin(), ng.end(), 0);
  g_raw = &rb;
  *n_runs = 0;
  const bool brk = std::getenv("K1B_HOST_BREAK_RUNS") != nullptr;  // (the test's own check: a run that starts one column late)
  for (int y = 0; y < rows;) {
    if (!active[y]) {
      ++y;
      continue;
    }
    int hi = y;
    while (hi + 1 < rows && active[hi + 1] && linked[hi + 1]) ++hi;
    const size_t off = (size_t)y * wb;
    std::vector<std::pair<int, int>> runs;
    {  // the kernel's way (the wave ORs a band's rows together): the rows' OR first, then column_runs_of_words
      std::vector<u64> occ(wb, 0);
      for (int r = 1; r <= hi - y + 1; ++r)
        for (int w = 0; w < wb; ++w) occ[w] |= nz[off + (size_t)r * wb + w];
      column_runs_of_words(occ.data(), wb, [&](int x0, int x1) { runs.push_back({x0, x1}); });
      if (wb <= 16) {  // ... and the lane-per-band form with the words in registers: the same runs
        std::vector<std::pair<int, int>> runs2;
        window_column_runs<16>(nz.data() + off, wb, hi - y + 1, [&](int x0, int x1) { runs2.push_back({x0, x1}); });
        if (runs2 != runs) return -1;
      }
    }
    // the runs in REVERSE order: the items of a band run on different lanes at once — no order may matter
    for (size_t k = runs.size(); k-- > 0;) {
      // ... each run cut again at the rows that are empty within its columns (window_run_rows), as the kernel does
      std::vector<std::pair<int, int>> sub;
      window_run_rows(nz.data() + off, wb, hi - y + 1, runs[k].first, runs[k].second,
                      [&](int first, int nrows) { sub.push_back({first, nrows}); });
      for (size_t q = sub.size(); q-- > 0;) {
        const int lo2 = y + sub[q].first - 1;
        const size_t off2 = (size_t)lo2 * wb;
        scan_window<true>(nz.data() + off2, pm.data() + off2, ng.data() + off2, wb, sub[q].second, lo2, 0, dp, 0, 0, &over,
                          [&](float mx, float my, unsigned key) { kb.push_back({mx, my, key}); },
                          runs[k].first + (brk ? 1 : 0), runs[k].second);
        ++*n_runs;
      }
    }
    y = hi + 1;
  }
  g_raw = nullptr;
  if (over) return -1;
  auto norm = [](std::vector<RawRec>& v) {
    std::sort(v.begin(), v.end(), [](const RawRec& a, const RawRec& b) { return a.key < b.key; });
  };
  norm(rw);
  norm(rb);
  if (rw.size() != rb.size()) return -1;
  for (size_t i = 0; i < rw.size(); ++i)
    if (rw[i].a00 != rb[i].a00 || rw[i].a10 != rb[i].a10 || rw[i].a01 != rb[i].a01 || rw[i].xmin != rb[i].xmin ||
        rw[i].xmax != rb[i].xmax || rw[i].ymin != rb[i].ymin || rw[i].ymax != rb[i].ymax || rw[i].key != rb[i].key)
      return -1;
  std::sort(kw.begin(), kw.end());
  std::sort(kb.begin(), kb.end());
  if (!(kw == kb)) return -1;
  return (int)rw.size();
}


// The general tier's blur on the RAW frame (PixWin::add + the image pass's flag bits: only flagged segments are loaded
// and thresholded, rows without one are skipped) against the blur on a thresholded copy of the frame (what the LDS
// tiers stage): the non-zero bitmaps must be identical.  Flags as the image pass sets them (any_gt16 per 16-byte
// segment).  Returns the number of set bitmap bits (>= 0), -1 on a mismatch.
extern "C" int host_blur_raw_vs_copy(const uint8_t* img, int rows, int cols, int thr, const int* taps, int ksize) {
  DetectParams dp;
  std::memset(&dp, 0, sizeof(dp));
  dp.thr = thr;
  dp.ksize = ksize;
  for (int i = 0; i < ksize; ++i) dp.taps[i] = taps[i];
  pack_taps(dp);
  const int nseg = (cols + 15) / 16, PW = 16 * nseg;
  std::vector<uint8_t> raw((size_t)rows * PW + 16, 0), pix;
  for (int y = 0; y < rows; ++y) std::memcpy(&raw[(size_t)y * PW], img + (size_t)y * cols, cols);
  pix = raw;
  const unsigned add = (unsigned)(255 - thr) * 0x00010001u;
  for (size_t i = 0; i + 4 <= pix.size(); i += 4) {
    unsigned w;
    std::memcpy(&w, &pix[i], 4);
    w = tozero4(w, add);
    std::memcpy(&pix[i], &w, 4);
  }
  const size_t fbit0 = 37;  // (a frame in the middle of a batch: its first segment is not word aligned)
  std::vector<u64> flags((fbit0 + (size_t)rows * nseg) / 64 + 2, 0);
  const ThrTest q = make_thr_test(thr);
  for (int y = 0; y < rows; ++y)
    for (int c = 0; c < nseg; ++c) {
      uint4 v;
      std::memcpy(&v, &raw[(size_t)y * PW + 16 * c], 16);
      if (any_gt16(v, q)) {
        const size_t g = fbit0 + (size_t)y * nseg + c;
        flags[g >> 6] |= 1ull << (g & 63);
      }
    }
  const int wb = (cols + 2 + 63) / 64 + 1;
  std::vector<u64> a((size_t)(rows + 2) * wb + 1, 0), b(a.size(), 0);
  const PixWin pc = {pix.data(), 0, rows, 0, PW, 0u, nullptr, 0};
  const PixWin pr = {raw.data(), 0, rows, 0, PW, add ? add : 1u, flags.data(), fbit0};
  for (int y = 0; y < rows; ++y)
    for (int c = 0; c < nseg; ++c) {
      blur_to_bitmap<false>(pc, rows, cols, dp, dp.taps, y, c, a.data() + (size_t)(y + 1) * wb, 0);
      if (add) blur_to_bitmap<true>(pr, rows, cols, dp, dp.taps, y, c, b.data() + (size_t)(y + 1) * wb, 0);
    }
  if (!add) return 0;
  int bits = 0;
  for (size_t i = 0; i < a.size(); ++i) {
    if (a[i] != b[i]) return -1;
    bits += __builtin_popcountll(a[i]);
  }
  return bits;
}
