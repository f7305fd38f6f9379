// gather_encoded_host.cpp — the segment arithmetic of k_gather_rois_encoded (csrc/mpe_gather.h, gather_segment_encoded)
// compiled for the HOST, as a stand-alone program that tests/test_encoded_device_streams.py builds with
// -fsanitize=address,undefined and runs.
//
// Seeded random cases per encoding (bgr8, rgb8, bgra8, rgba8, mono16 little- and big-endian): an image of 1 x 1 ..
// 24 x 40 pixels with stride = cols * bpp + {0, 1, 3, 16}, based 0 .. 3 bytes into a heap buffer that ends with the
// image's last byte, a ROI (whole image, a corner, widths 1 .. 17, widths that are no multiple of 16) and a slot at
// least as large as the ROI.  Every slot must equal a per-pixel conversion written out here (the two formulas of
// include/mpe.h in scalar code of this file's own, not csrc/mpe_pixel.h) plus zero fill.  The no-over-read invariant
// is checked twice: AddressSanitizer sees any load behind the buffer, and the loads themselves (CheckedLoads) refuse an
// address outside the image or an unaligned dword — that also covers the bytes in FRONT of an image whose base is not
// the start of the allocation, which the sanitizer cannot see.
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
  mutable long n32 = 0, n8 = 0;
  uint32_t ld32(uintptr_t a) const {
    if (a < lo || a + 4 > hi || (a & 3)) {
      std::fprintf(stderr, "dword load outside the image or unaligned: offset %ld of %ld\n", (long)(a - lo), (long)(hi - lo));
      std::abort();
    }
    ++n32;
    uint32_t v;
    std::memcpy(&v, reinterpret_cast<const void*>(a), 4);
    return v;
  }
  uint32_t ld8(uintptr_t a) const {
    if (a < lo || a >= hi) {
      std::fprintf(stderr, "byte load outside the image: offset %ld of %ld\n", (long)(a - lo), (long)(hi - lo));
      std::abort();
    }
    ++n8;
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

// one pixel, plainly: Y = (B * 1868 + G * 9617 + R * 4899 + 2^13) >> 14, and round-half-even of the single-precision
// product v * (float)(255 / 65535), clamped
uint8_t convert_px(const uint8_t* p, const Encoding& e) {
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

template <int BPP>
int run(const Encoding& e, int n_cases) {
  const int strides[4] = {0, 1, 3, 16};
  long segments = 0, dwords = 0, bytes = 0;
  int kinds[6] = {0, 0, 0, 0, 0, 0};
  for (int c = 0; c < n_cases; ++c) {
    const int rows = c % 97 == 0 ? 1 : rnd_in(1, 24), cols = c % 89 == 0 ? 1 : rnd_in(1, 40);
    const size_t stride = (size_t)cols * BPP + strides[rnd() % 4];
    const int off = (int)(rnd() % 4);
    const size_t img_bytes = (size_t)(rows - 1) * stride + (size_t)cols * BPP;
    // the allocation ends with the image's last byte
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(off + img_bytes));
    for (size_t i = 0; i < off + img_bytes; ++i) buf[i] = (uint8_t)rnd();
    const uint8_t* img = buf + off;
    int x, y, w, h;
    const int kind = c % 6;
    ++kinds[kind];
    if (kind == 0) {  // the whole image
      x = y = 0;
      w = cols;
      h = rows;
    } else {
      w = rnd_in(1, kind == 1 && cols > 17 ? 17 : cols);  // (kind 1: widths 1 .. 17)
      if (kind == 2 && w % 16 == 0) --w;  // no multiple of 16
      h = rnd_in(1, rows);
      if (kind <= 4) {  // one of the four corners (by c / 6)
        x = (c / 6) & 1 ? cols - w : 0;
        y = (c / 6) & 2 ? rows - h : 0;
      } else {
        x = rnd_in(0, cols - w);
        y = rnd_in(0, rows - h);
      }
    }
    // a slot at least as large as the ROI, its pitch a multiple of 16
    const int g_rows = h + rnd_in(0, 3), pitch = ((w + 15) / 16 + (int)(rnd() % 2)) * 16;
    std::vector<uint8_t> want((size_t)g_rows * pitch, 0), got((size_t)g_rows * pitch, 0xee);
    for (int r = 0; r < h; ++r)
      for (int q = 0; q < w; ++q)
        want[(size_t)r * pitch + q] = convert_px(img + (size_t)(y + r) * stride + (size_t)(x + q) * BPP, e);
    CheckedLoads mem{reinterpret_cast<uintptr_t>(img), reinterpret_cast<uintptr_t>(img) + img_bytes};
    for (int r = 0; r < g_rows; ++r)
      for (int seg = 0; seg < pitch / 16; ++seg) {
        uint32_t o[4];
        mpe::gather_segment_encoded<BPP>(mem, img, img_bytes, stride, x, y, w, h, r, seg, e.rgb, e.big_endian, o);
        std::memcpy(&got[(size_t)r * pitch + 16 * seg], o, 16);
        ++segments;
      }
    dwords += mem.n32;
    bytes += mem.n8;
    if (got != want) {
      size_t i = 0;
      while (got[i] == want[i]) ++i;
      std::fprintf(stderr, "%s case %d: image %d x %d stride %zu base +%d, ROI %d %d %d %d, slot %d x %d: byte %zu (row %zu, "
                   "column %zu) is %u, expected %u\n", e.name, c, rows, cols, stride, off, x, y, w, h, g_rows, pitch, i,
                   i / pitch, i % pitch, got[i], want[i]);
      return 1;
    }
    // the plain loads give the same bytes (what the kernel instantiates)
    for (int r = 0; r < g_rows; r += 3) {
      uint32_t o[4];
      mpe::gather_segment_encoded<BPP>(mpe::GatherLoads(), img, img_bytes, stride, x, y, w, h, r, 0, e.rgb, e.big_endian, o);
      if (std::memcmp(o, &want[(size_t)r * pitch], 16)) {
        std::fprintf(stderr, "%s case %d: plain loads differ in row %d\n", e.name, c, r);
        return 1;
      }
    }
    std::free(buf);
  }
  std::printf("gather_encoded_host ok: %s %d cases (whole %d, narrow %d, odd width %d, corner %d + %d, inside %d), %ld segments, "
              "%ld dword loads, %ld byte loads\n", e.name, n_cases, kinds[0], kinds[1], kinds[2], kinds[3], kinds[4], kinds[5],
              segments, dwords, bytes);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const int n_cases = argc > 1 ? std::atoi(argv[1]) : 2000;
  // every 16-bit value against the mono16 rule, both byte orders, through a one-pixel image
  for (unsigned v = 0; v < 65536; ++v) {
    const uint8_t le[2] = {(uint8_t)(v & 255), (uint8_t)(v >> 8)}, be[2] = {(uint8_t)(v >> 8), (uint8_t)(v & 255)};
    const Encoding e_le = {"mono16", 2, false, false}, e_be = {"mono16 big-endian", 2, false, true};
    uint32_t o[4], p[4];
    mpe::gather_segment_encoded<2>(mpe::GatherLoads(), le, 2, 2, 0, 0, 1, 1, 0, 0, false, false, o);
    mpe::gather_segment_encoded<2>(mpe::GatherLoads(), be, 2, 2, 0, 0, 1, 1, 0, 0, false, true, p);
    if (o[0] != convert_px(le, e_le) || p[0] != convert_px(be, e_be) || o[0] != p[0] || o[1] || o[2] || o[3]) {
      std::fprintf(stderr, "mono16 value %u: %u / %u, expected %u\n", v, o[0], p[0], convert_px(le, e_le));
      return 1;
    }
  }
  const Encoding encs[6] = {{"bgr8", 3, false, false},  {"rgb8", 3, true, false},    {"bgra8", 4, false, false},
                            {"rgba8", 4, true, false},  {"mono16", 2, false, false}, {"mono16 big-endian", 2, false, true}};
  for (const Encoding& e : encs) {
    const int rc = e.bpp == 2 ? run<2>(e, n_cases) : (e.bpp == 3 ? run<3>(e, n_cases) : run<4>(e, n_cases));
    if (rc) return rc;
  }
  return 0;
}
