// gather_formats_host.cpp — the segment arithmetic of k_gather_rois_formats (csrc/mpe_gather.h, gather_segment_format)
// compiled for the HOST, as a stand-alone program that tests/test_mixed_format_streams.py builds with
// -fsanitize=address,undefined and runs.
//
// Seeded random cases.  A case is ONE submission: a table of 2 .. 6 items whose image formats are drawn from the seven
// variants (mono8, bgr8, rgb8, bgra8, rgba8, mono16 little- and big-endian), a format table that holds every distinct
// format once, and one slot geometry for all items (the largest ROI of the case, sometimes larger).  Every image has
// 1 x 1 .. 24 x 40 pixels, stride = cols * bpp + {0, 1, 3, 16}, and sits 0 .. 3 bytes into a heap buffer OF ITS OWN that
// ends with the image's last byte.  ROIs: the whole image, a corner, widths 1 .. 17, widths that are no multiple of 16,
// anywhere inside.  Item 0 is smaller than item 1 in both directions and its ROI lies at the far corner of its own
// image: one pixel further right or down it would still fit item 1's image, so a segment that took the size, stride or
// end of another item's format reads outside item 0's buffer.  The slots are computed as the kernel computes them
// (segment index -> item, row, segment; the item's entry of the format table) and every slot must equal a per-pixel
// conversion written out here (the two formulas of include/mpe.h in scalar code of this file's own) plus zero fill.
// The no-over-read invariant is checked twice: AddressSanitizer sees any load behind a buffer, and the loads themselves
// (CheckedLoads, against the item's own image) refuse an address outside the image or an unaligned dword.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>  // tests/host/stub
#include "mpe_gather.h"

namespace {

struct CheckedLoads {
  uintptr_t lo, hi;
  long* n32;
  long* n8;
  uint32_t ld32(uintptr_t a) const {
    if (a < lo || a + 4 > hi || (a & 3)) {
      std::fprintf(stderr, "dword load outside the image or unaligned: offset %ld of %ld\n", (long)(a - lo), (long)(hi - lo));
      std::abort();
    }
    ++*n32;
    uint32_t v;
    std::memcpy(&v, reinterpret_cast<const void*>(a), 4);
    return v;
  }
  uint32_t ld8(uintptr_t a) const {
    if (a < lo || a >= hi) {
      std::fprintf(stderr, "byte load outside the image: offset %ld of %ld\n", (long)(a - lo), (long)(hi - lo));
      std::abort();
    }
    ++*n8;
    return *reinterpret_cast<const uint8_t*>(a);
  }
};

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}
int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }  // inclusive

struct Encoding {
  const char* name;
  int bpp;
  bool rgb, big_endian;
};
const Encoding kEncodings[7] = {{"mono8", 1, false, false}, {"bgr8", 3, false, false},   {"rgb8", 3, true, false},
                                {"bgra8", 4, false, false}, {"rgba8", 4, true, false},   {"mono16", 2, false, false},
                                {"mono16 big-endian", 2, false, true}};

// one pixel, plainly: Y = (B * 1868 + G * 9617 + R * 4899 + 2^13) >> 14, and round-half-even of the single-precision
// product v * (float)(255 / 65535), clamped
uint8_t convert_px(const uint8_t* p, const Encoding& e) {
  if (e.bpp == 1) return p[0];
  if (e.bpp == 2) {
    const unsigned v = e.big_endian ? (unsigned)p[0] * 256u + p[1] : (unsigned)p[1] * 256u + p[0];
    const float scale = (float)(255.0 / 65535.0);
    float y = std::nearbyintf((float)v * scale);  // (the default rounding mode: to nearest, ties to even)
    if (y < 0.f) y = 0.f;
    if (y > 255.f) y = 255.f;
    return (uint8_t)y;
  }
  const unsigned blue = e.rgb ? p[2] : p[0], green = p[1], red = e.rgb ? p[0] : p[2];
  return (uint8_t)((blue * 1868u + green * 9617u + red * 4899u + 8192u) >> 14);
}

struct Image {
  int enc, rows, cols, off;
  size_t stride, img_bytes;
  uint8_t* buf;
  const uint8_t* img;
  int x, y, w, h;
};

}  // namespace

int main(int argc, char** argv) {
  const int n_cases = argc > 1 ? std::atoi(argv[1]) : 2000;
  const int strides[4] = {0, 1, 3, 16};
  long items = 0, segments = 0, dwords = 0, bytes = 0, tables = 0, far_corner = 0;
  int per_enc[7] = {0, 0, 0, 0, 0, 0, 0}, kinds[6] = {0, 0, 0, 0, 0, 0};
  for (int c = 0; c < n_cases; ++c) {
    const int n = rnd_in(2, 6);
    std::vector<Image> im((size_t)n);
    for (int i = 0; i < n; ++i) {
      Image& m = im[(size_t)i];
      m.enc = (int)(rnd() % 7);
      if (i == 0) {  // smaller than item 1 in both directions
        m.rows = c % 97 == 0 ? 1 : rnd_in(1, 23);
        m.cols = c % 89 == 0 ? 1 : rnd_in(1, 39);
      } else if (i == 1) {
        m.rows = rnd_in(im[0].rows + 1, 24);
        m.cols = rnd_in(im[0].cols + 1, 40);
      } else {
        m.rows = rnd_in(1, 24);
        m.cols = rnd_in(1, 40);
      }
      const int bpp = kEncodings[m.enc].bpp;
      m.stride = (size_t)m.cols * bpp + strides[rnd() % 4];
      m.off = (int)(rnd() % 4);
      m.img_bytes = (size_t)(m.rows - 1) * m.stride + (size_t)m.cols * bpp;
      m.buf = static_cast<uint8_t*>(std::malloc(m.off + m.img_bytes));  // ends with the image's last byte
      for (size_t k = 0; k < m.off + m.img_bytes; ++k) m.buf[k] = (uint8_t)rnd();
      m.img = m.buf + m.off;
      const int kind = i == 0 ? 4 : (c + i) % 6;
      ++kinds[kind];
      if (kind == 0) {  // the whole image
        m.x = m.y = 0;
        m.w = m.cols;
        m.h = m.rows;
      } else {
        m.w = rnd_in(1, kind == 1 && m.cols > 17 ? 17 : m.cols);  // (kind 1: widths 1 .. 17)
        if (kind == 2 && m.w % 16 == 0) --m.w;                     // no multiple of 16
        if (m.w < 1) m.w = 1;
        m.h = rnd_in(1, m.rows);
        if (i == 0) {  // the far corner of its own image
          m.x = m.cols - m.w;
          m.y = m.rows - m.h;
          ++far_corner;
        } else if (kind <= 4) {  // one of the four corners (by c / 6)
          m.x = (c / 6) & 1 ? m.cols - m.w : 0;
          m.y = (c / 6) & 2 ? m.rows - m.h : 0;
        } else {
          m.x = rnd_in(0, m.cols - m.w);
          m.y = rnd_in(0, m.rows - m.h);
        }
      }
      ++per_enc[m.enc];
    }
    // (the premise of the far-corner item: shifted by one pixel its ROI leaves its own image and stays inside item 1's)
    if (im[0].x + 1 + im[0].w > im[1].cols || im[0].y + 1 + im[0].h > im[1].rows) {
      std::fprintf(stderr, "case %d: item 0's ROI does not fit item 1's image\n", c);
      return 1;
    }
    // the submission: one slot geometry, the items in shuffled slot order, every distinct format once
    int g_rows = 0, wmax = 0;
    for (const Image& m : im) {
      g_rows = m.h > g_rows ? m.h : g_rows;
      wmax = m.w > wmax ? m.w : wmax;
    }
    g_rows += rnd_in(0, 3);
    const int segs_per_row = (wmax + 15) / 16 + (int)(rnd() % 2), pitch = 16 * segs_per_row;
    const size_t slot_bytes = (size_t)g_rows * pitch;
    std::vector<int> slot_of((size_t)n);
    for (int i = 0; i < n; ++i) slot_of[(size_t)i] = i;
    for (int i = n - 1; i > 0; --i) std::swap(slot_of[(size_t)i], slot_of[(size_t)(rnd() % (uint32_t)(i + 1))]);
    std::vector<mpe::GatherFormat> fmts;
    std::vector<mpe::GatherItem> tab((size_t)n);
    std::vector<int> item_of_slot((size_t)n);
    for (int i = 0; i < n; ++i) {
      const Image& m = im[(size_t)i];
      const Encoding& e = kEncodings[m.enc];
      const mpe::GatherFormat f = {m.stride, m.img_bytes, e.bpp, e.rgb ? 1 : 0, e.big_endian ? 1 : 0, 0};
      size_t k = 0;
      while (k < fmts.size() && std::memcmp(&fmts[k], &f, sizeof(f))) ++k;
      if (k == fmts.size()) fmts.push_back(f);
      const int s = slot_of[(size_t)i];
      tab[(size_t)s] = mpe::GatherItem{m.img, m.x, m.y, m.w, m.h, s, (int)k};
      item_of_slot[(size_t)s] = i;
    }
    tables += (long)fmts.size();
    std::vector<uint8_t> want((size_t)n * slot_bytes, 0), got((size_t)n * slot_bytes, 0xee);
    for (int i = 0; i < n; ++i) {
      const Image& m = im[(size_t)i];
      uint8_t* slot = &want[(size_t)slot_of[(size_t)i] * slot_bytes];
      for (int r = 0; r < m.h; ++r)
        for (int q = 0; q < m.w; ++q)
          slot[(size_t)r * pitch + q] =
              convert_px(m.img + (size_t)(m.y + r) * m.stride + (size_t)(m.x + q) * kEncodings[m.enc].bpp, kEncodings[m.enc]);
    }
    // what k_gather_rois_formats does with segment idx
    const size_t segs_per_slot = (size_t)g_rows * segs_per_row;
    for (size_t idx = 0; idx < (size_t)n * segs_per_slot; ++idx) {
      const int e = (int)(idx / segs_per_slot);
      const int rem = (int)(idx - (size_t)e * segs_per_slot);
      const int r = rem / segs_per_row, seg = rem - r * segs_per_row;
      const mpe::GatherItem it = tab[(size_t)e];
      const mpe::GatherFormat f = fmts[(size_t)it.format];
      const Image& m = im[(size_t)item_of_slot[(size_t)e]];
      const CheckedLoads mem{reinterpret_cast<uintptr_t>(m.img), reinterpret_cast<uintptr_t>(m.img) + m.img_bytes, &dwords,
                             &bytes};
      uint32_t o[4];
      mpe::gather_segment_format(mem, it.img, f, it.x, it.y, it.w, it.h, r, seg, o);
      std::memcpy(&got[(size_t)it.slot * slot_bytes + ((size_t)r * segs_per_row + seg) * 16], o, 16);
      ++segments;
    }
    if (got != want) {
      size_t k = 0;
      while (got[k] == want[k]) ++k;
      const Image& m = im[(size_t)item_of_slot[k / slot_bytes]];
      std::fprintf(stderr, "case %d, slot %zu (%s): image %d x %d stride %zu base +%d, ROI %d %d %d %d, slot %d x %d: byte %zu "
                   "is %u, expected %u\n", c, k / slot_bytes, kEncodings[m.enc].name, m.rows, m.cols, m.stride, m.off, m.x,
                   m.y, m.w, m.h, g_rows, pitch, k % slot_bytes, got[k], want[k]);
      return 1;
    }
    // the plain loads give the same bytes (what the kernel instantiates)
    for (int e = 0; e < n; ++e) {
      const mpe::GatherItem it = tab[(size_t)e];
      uint32_t o[4];
      mpe::gather_segment_format(mpe::GatherLoads(), it.img, fmts[(size_t)it.format], it.x, it.y, it.w, it.h, 0, 0, o);
      if (std::memcmp(o, &want[(size_t)e * slot_bytes], 16)) {
        std::fprintf(stderr, "case %d: plain loads differ in slot %d\n", c, e);
        return 1;
      }
    }
    items += n;
    for (Image& m : im) std::free(m.buf);
  }
  std::printf("gather_formats_host ok: %d cases, %ld items (mono8 %d, bgr8 %d, rgb8 %d, bgra8 %d, rgba8 %d, mono16 %d, mono16 "
              "big-endian %d), %ld format table entries, %ld far-corner items, ROIs (whole %d, narrow %d, odd width %d, "
              "corner %d + %d, inside %d), %ld segments, %ld dword loads, %ld byte loads\n", n_cases, items, per_enc[0],
              per_enc[1], per_enc[2], per_enc[3], per_enc[4], per_enc[5], per_enc[6], tables, far_corner, kinds[0], kinds[1],
              kinds[2], kinds[3], kinds[4], kinds[5], segments, dwords, bytes);
  return 0;
}
