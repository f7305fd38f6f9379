// gather_host.cpp — the segment arithmetic of k_gather_rois (csrc/mpe_gather.h) compiled for the HOST, as a stand-alone
// program that tests/test_device_frame_streams.py builds with -fsanitize=address,undefined and runs.
//
// Seeded random cases: an image of 1 x 1 .. 48 x 64 pixels with stride = cols + {0, 1, 3, 16}, based 0 .. 3 bytes
// into a heap buffer that ends with the image's last pixel, a ROI (whole image, a corner, widths 1 .. 17, widths that
// are no multiple of 16) and a slot at least as large as the ROI.  Every slot must equal a per-byte copy plus zero
// fill.  The no-over-read invariant is checked twice: AddressSanitizer sees any load behind the buffer, and the loads
// themselves (CheckedLoads) refuse an address outside the image — that also covers the bytes in FRONT of an image
// whose base is not the start of the allocation, which the sanitizer cannot see.
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

}  // namespace

int main(int argc, char** argv) {
  const int n_cases = argc > 1 ? std::atoi(argv[1]) : 2000;
  const int strides[4] = {0, 1, 3, 16};
  long segments = 0, dwords = 0, bytes = 0;
  int kinds[6] = {0, 0, 0, 0, 0, 0};
  for (int c = 0; c < n_cases; ++c) {
    const int rows = c % 97 == 0 ? 1 : rnd_in(1, 48), cols = c % 89 == 0 ? 1 : rnd_in(1, 64);
    const size_t stride = (size_t)cols + strides[rnd() % 4];
    const int off = (int)(rnd() % 4);
    const size_t img_bytes = (size_t)(rows - 1) * stride + cols;
    // the allocation ends with the image's last pixel
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(off + img_bytes));
    for (size_t i = 0; i < off + img_bytes; ++i) buf[i] = (uint8_t)(1 + rnd() % 255);  // (never zero: a missed byte shows)
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
      for (int q = 0; q < w; ++q) want[(size_t)r * pitch + q] = img[(size_t)(y + r) * stride + x + q];
    CheckedLoads mem{reinterpret_cast<uintptr_t>(img), reinterpret_cast<uintptr_t>(img) + img_bytes};
    for (int r = 0; r < g_rows; ++r)
      for (int seg = 0; seg < pitch / 16; ++seg) {
        uint32_t o[4];
        mpe::gather_segment(mem, img, img_bytes, stride, x, y, w, h, r, seg, o);
        std::memcpy(&got[(size_t)r * pitch + 16 * seg], o, 16);
        ++segments;
      }
    dwords += mem.n32;
    bytes += mem.n8;
    if (got != want) {
      size_t i = 0;
      while (got[i] == want[i]) ++i;
      std::fprintf(stderr, "case %d: image %d x %d stride %zu base +%d, ROI %d %d %d %d, slot %d x %d: byte %zu (row %zu, "
                   "column %zu) is %u, expected %u\n", c, rows, cols, stride, off, x, y, w, h, g_rows, pitch, i, i / pitch,
                   i % pitch, got[i], want[i]);
      return 1;
    }
    // the plain loads give the same bytes (what the kernel instantiates)
    for (int r = 0; r < g_rows; r += 3) {
      uint32_t o[4];
      mpe::gather_segment(mpe::GatherLoads(), img, img_bytes, stride, x, y, w, h, r, 0, o);
      if (std::memcmp(o, &want[(size_t)r * pitch], 16)) {
        std::fprintf(stderr, "case %d: plain loads differ in row %d\n", c, r);
        return 1;
      }
    }
    std::free(buf);
  }
  std::printf("gather_host ok: %d cases (whole %d, narrow %d, odd width %d, corner %d + %d, inside %d), %ld segments, "
              "%ld dword loads, %ld byte loads\n", n_cases, kinds[0], kinds[1], kinds[2], kinds[3], kinds[4], kinds[5],
              segments, dwords, bytes);
  return 0;
}
