// gather_sensor_host.cpp — the segment arithmetic of the Bayer and YUV 4:2:2 gathers (csrc/mpe_gather.h:
// gather_segment_bayer, gather_segment_yuv, and gather_segment_format over tables that hold such entries) compiled for
// the HOST, as a stand-alone program that tests/test_sensor_encodings.py builds with -fsanitize=address,undefined and
// runs.
//
// Part 1, per encoding (bayer_rggb8, bayer_bggr8, bayer_gbrg8, bayer_grbg8, yuv422, yuv422_yuy2): seeded random cases.
// Images of 1 x 1 .. 24 x 40 pixels (so rows < 3 and cols < 3 occur), stride = cols * bpp + {0, 1, 3, 16}, the image
// 0 .. 3 bytes into a heap buffer that ends with the image's last byte.  ROIs: the whole image, each corner, odd and even
// origins, widths 1 .. 17, widths that are no multiple of 16, anywhere inside; slots larger than the ROI.  Every slot
// is compared byte for byte with this file's own per-pixel decode of the WHOLE image (a colour-map statement of the
// rule of include/mpe.h: every neighbour weighted by the weight of the colour the pattern gives it, then the border
// rows and columns filled from their inner neighbours) cut to the ROI, plus zero fill.
// Part 2: submissions whose items mix mono8, bgr8, the four Bayer patterns and the two YUV orders, through
// gather_segment_format with a format table as submit_slots (mpe_track_abi.cpp) writes it.
// The no-over-read invariant is checked twice: AddressSanitizer sees any load behind a buffer, and the loads themselves
// (CheckedLoads, against the item's own image) refuse an address outside the image or an unaligned dword.
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
  int code, bpp;
  const char* pattern;  // Bayer: the colours of the pixels (0,0), (0,1), (1,0), (1,1)
  int y_byte;           // YUV: which byte of a pixel's two
  bool rgb;
};
const Encoding kEncodings[8] = {
    {"bayer_rggb8", MPE_ENC_BAYER_RGGB8, 1, "RGGB", 0, false}, {"bayer_bggr8", MPE_ENC_BAYER_BGGR8, 1, "BGGR", 0, false},
    {"bayer_gbrg8", MPE_ENC_BAYER_GBRG8, 1, "GBRG", 0, false}, {"bayer_grbg8", MPE_ENC_BAYER_GRBG8, 1, "GRBG", 0, false},
    {"yuv422", MPE_ENC_YUV422, 2, nullptr, 1, false},          {"yuv422_yuy2", MPE_ENC_YUV422_YUY2, 2, nullptr, 0, false},
    {"mono8", MPE_ENC_MONO8, 1, nullptr, 0, false},            {"bgr8", MPE_ENC_BGR8, 3, nullptr, 0, false}};

unsigned weight(char colour) { return colour == 'R' ? 4899u : (colour == 'G' ? 9617u : 1868u); }

// the whole image, plainly -> rows x cols bytes
std::vector<uint8_t> decode_image(const uint8_t* img, int rows, int cols, size_t stride, const Encoding& e) {
  std::vector<uint8_t> out((size_t)rows * cols, 0);
  auto at = [&](int y, int x) { return (unsigned)img[(size_t)y * stride + (size_t)x]; };
  if (!e.pattern) {
    for (int y = 0; y < rows; ++y)
      for (int x = 0; x < cols; ++x) {
        const uint8_t* p = img + (size_t)y * stride + (size_t)x * e.bpp;
        out[(size_t)y * cols + x] = e.bpp == 1   ? p[0]
                                    : e.bpp == 2 ? p[e.y_byte]
                                                 : (uint8_t)((p[0] * 1868u + p[1] * 9617u + p[2] * 4899u + 8192u) >> 14);
      }
    return out;
  }
  if (rows < 3 || cols < 3) return out;
  auto colour = [&](int y, int x) { return e.pattern[2 * (y & 1) + (x & 1)]; };
  for (int y = 1; y < rows - 1; ++y)
    for (int x = 1; x < cols - 1; ++x) {
      const unsigned c = at(y, x);
      unsigned acc;
      if (colour(y, x) == 'G') {
        acc = weight(colour(y - 1, x)) * at(y - 1, x) + weight(colour(y + 1, x)) * at(y + 1, x) +
              weight(colour(y, x - 1)) * at(y, x - 1) + weight(colour(y, x + 1)) * at(y, x + 1) + 2u * 9617u * c + (1u << 14);
        acc >>= 15;
      } else {
        acc = 0;
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx)
            if (dy || dx) acc += weight(colour(y + dy, x + dx)) * at(y + dy, x + dx);
        acc += 4u * weight(colour(y, x)) * c + (1u << 15);
        acc >>= 16;
      }
      out[(size_t)y * cols + x] = (uint8_t)acc;
    }
  for (int y = 1; y < rows - 1; ++y) {  // the first and last column, then the first and last row (corners with them)
    out[(size_t)y * cols] = out[(size_t)y * cols + 1];
    out[(size_t)y * cols + cols - 1] = out[(size_t)y * cols + cols - 2];
  }
  for (int x = 0; x < cols; ++x) {
    out[(size_t)x] = out[(size_t)cols + x];
    out[(size_t)(rows - 1) * cols + x] = out[(size_t)(rows - 2) * cols + x];
  }
  return out;
}

struct Image {
  int enc, rows, cols, off;
  size_t stride, img_bytes;
  uint8_t* buf;
  const uint8_t* img;
  int x, y, w, h;
  std::vector<uint8_t> mono;
};

// image c of a run: size, stride, base, pixels, ROI of kind `kind` (0 whole, 1 narrow, 2 no multiple of 16, 3 / 4 a
// corner by `corner`, 5 anywhere, 6 anywhere at an odd origin, 7 anywhere at an even origin)
void make_image(Image& m, int enc, int c, int kind, int corner) {
  const int strides[4] = {0, 1, 3, 16};
  const Encoding& e = kEncodings[enc];
  m.enc = enc;
  m.rows = c % 97 == 0 ? 1 : (c % 53 == 0 ? 2 : rnd_in(1, 24));
  m.cols = c % 89 == 0 ? 1 : (c % 59 == 0 ? 2 : rnd_in(1, 40));
  m.stride = (size_t)m.cols * e.bpp + strides[rnd() % 4];
  m.off = (int)(rnd() % 4);
  m.img_bytes = (size_t)(m.rows - 1) * m.stride + (size_t)m.cols * e.bpp;
  m.buf = static_cast<uint8_t*>(std::malloc(m.off + m.img_bytes));  // ends with the image's last byte
  for (size_t k = 0; k < m.off + m.img_bytes; ++k) m.buf[k] = (uint8_t)rnd();
  m.img = m.buf + m.off;
  m.mono = decode_image(m.img, m.rows, m.cols, m.stride, e);
  if (kind == 0) {
    m.x = m.y = 0;
    m.w = m.cols;
    m.h = m.rows;
    return;
  }
  m.w = rnd_in(1, kind == 1 && m.cols > 17 ? 17 : m.cols);
  if (kind == 2 && m.w % 16 == 0) --m.w;
  if (m.w < 1) m.w = 1;
  m.h = rnd_in(1, m.rows);
  if (kind <= 4) {
    m.x = corner & 1 ? m.cols - m.w : 0;
    m.y = corner & 2 ? m.rows - m.h : 0;
  } else {
    m.x = rnd_in(0, m.cols - m.w);
    m.y = rnd_in(0, m.rows - m.h);
    if (kind >= 6) {  // the wanted parity where the image has room for it
      const int par = kind == 6 ? 1 : 0;
      if ((m.x & 1) != par) m.x += m.x + 1 + m.w <= m.cols ? 1 : (m.x > 0 ? -1 : 0);
      if ((m.y & 1) != par) m.y += m.y + 1 + m.h <= m.rows ? 1 : (m.y > 0 ? -1 : 0);
    }
  }
}

mpe::GatherFormat format_of(const Image& m) {  // as submit_slots writes the entry
  const Encoding& e = kEncodings[m.enc];
  mpe::GatherFormat f = {m.stride, m.img_bytes, e.bpp, 0, 0, mpe::encoding_kind(e.code)};
  if (f.kind == mpe::PIX_YUV) f.big_endian = mpe::yuv_y_byte(e.code);
  if (f.kind == mpe::PIX_BAYER) {
    f.rgb = m.cols;
    f.big_endian = m.rows;
    f.kind = mpe::PIX_BAYER | (mpe::bayer_phase(e.code) << 8);
  }
  return f;
}

void want_slot(const Image& m, uint8_t* slot, int pitch) {  // (zero-filled before)
  for (int r = 0; r < m.h; ++r)
    for (int q = 0; q < m.w; ++q) slot[(size_t)r * pitch + q] = m.mono[(size_t)(m.y + r) * m.cols + (m.x + q)];
}

int report(const char* what, int c, const Image& m, int g_rows, int pitch, size_t k, unsigned got, unsigned want) {
  std::fprintf(stderr, "%s case %d (%s): image %d x %d stride %zu base +%d, ROI %d %d %d %d, slot %d x %d: byte %zu is %u, "
               "expected %u\n", what, c, kEncodings[m.enc].name, m.rows, m.cols, m.stride, m.off, m.x, m.y, m.w, m.h, g_rows,
               pitch, k, got, want);
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  const int n_cases = argc > 1 ? std::atoi(argv[1]) : 2000;
  // ---- the codes every entry checks its `encoding` with: bytes per pixel and kind, 0 for anything outside MPE_ENC_*
  for (int code = -2; code <= 24; ++code) {
    int bpp = 0, kind = mpe::PIX_NONE;
    if (code >= 0 && code <= 5) {
      const int plain[6] = {1, 3, 3, 4, 4, 2};
      bpp = plain[code];
      kind = mpe::PIX_PLAIN;
    } else if (code >= 16 && code <= 19) {
      bpp = 1;
      kind = mpe::PIX_BAYER;
    } else if (code == 20 || code == 21) {
      bpp = 2;
      kind = mpe::PIX_YUV;
    }
    if (mpe::encoding_bytes_per_pixel(code) != bpp || mpe::encoding_kind(code) != kind) {
      std::fprintf(stderr, "encoding %d: %d bytes per pixel, kind %d\n", code, mpe::encoding_bytes_per_pixel(code),
                   mpe::encoding_kind(code));
      return 1;
    }
  }
  std::printf("gather_sensor_host ok: encodings -2 .. 24\n");
  // ---- part 1: one image per case, the segment function of its family called as the kernels call it
  for (int enc = 0; enc < 6; ++enc) {
    const Encoding& e = kEncodings[enc];
    long segments = 0, dwords = 0, bytes = 0, small = 0, odd = 0;
    for (int c = 0; c < n_cases; ++c) {
      Image m;
      make_image(m, enc, c, c % 8, c / 8);
      small += m.rows < 3 || m.cols < 3;
      odd += (m.x & 1) || (m.y & 1);
      const int g_rows = m.h + rnd_in(0, 3);
      const int segs_per_row = (m.w + 15) / 16 + (int)(rnd() % 2), pitch = 16 * segs_per_row;
      std::vector<uint8_t> want((size_t)g_rows * pitch, 0), got((size_t)g_rows * pitch, 0xee);
      want_slot(m, want.data(), pitch);
      const CheckedLoads mem{reinterpret_cast<uintptr_t>(m.img), reinterpret_cast<uintptr_t>(m.img) + m.img_bytes, &dwords,
                             &bytes};
      for (int r = 0; r < g_rows; ++r)
        for (int seg = 0; seg < segs_per_row; ++seg) {
          uint32_t o[4];
          if (e.pattern)
            mpe::gather_segment_bayer(mem, m.img, m.img_bytes, m.stride, m.rows, m.cols, m.x, m.y, m.w, m.h, r, seg,
                                      mpe::bayer_phase(e.code), o);
          else
            mpe::gather_segment_yuv(mem, m.img, m.img_bytes, m.stride, m.x, m.y, m.w, m.h, r, seg, mpe::yuv_y_byte(e.code), o);
          std::memcpy(&got[((size_t)r * segs_per_row + seg) * 16], o, 16);
          ++segments;
        }
      if (got != want) {
        size_t k = 0;
        while (got[k] == want[k]) ++k;
        return report("segment", c, m, g_rows, pitch, k, got[k], want[k]);
      }
      {  // the plain loads give the same bytes (what the kernels instantiate)
        uint32_t o[4];
        if (e.pattern)
          mpe::gather_segment_bayer(mpe::GatherLoads(), m.img, m.img_bytes, m.stride, m.rows, m.cols, m.x, m.y, m.w, m.h,
                                    m.h - 1, (m.w - 1) / 16, mpe::bayer_phase(e.code), o);
        else
          mpe::gather_segment_yuv(mpe::GatherLoads(), m.img, m.img_bytes, m.stride, m.x, m.y, m.w, m.h, m.h - 1,
                                  (m.w - 1) / 16, mpe::yuv_y_byte(e.code), o);
        if (std::memcmp(o, &want[((size_t)(m.h - 1) * segs_per_row + (m.w - 1) / 16) * 16], 16)) {
          std::fprintf(stderr, "%s case %d: plain loads differ\n", e.name, c);
          return 1;
        }
      }
      std::free(m.buf);
    }
    std::printf("gather_sensor_host ok: %s %d cases (%ld below 3 x 3, %ld odd origins), %ld segments, %ld dword loads, %ld byte "
                "loads\n", e.name, n_cases, small, odd, segments, dwords, bytes);
  }
  // ---- part 2: submissions that mix mono8, bgr8, Bayer and YUV items, through the format table
  long items = 0, segments = 0, dwords = 0, bytes = 0, tables = 0;
  int per_enc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int c = 0; c < n_cases; ++c) {
    const int n = rnd_in(2, 6);
    std::vector<Image> im((size_t)n);
    for (int i = 0; i < n; ++i) {
      make_image(im[(size_t)i], i < 4 ? (c + 3 * i) % 8 : (int)(rnd() % 8), c + i, (c + i) % 8, c / 8);
      ++per_enc[im[(size_t)i].enc];
    }
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
    std::vector<uint8_t> want((size_t)n * slot_bytes, 0), got((size_t)n * slot_bytes, 0xee);
    for (int i = 0; i < n; ++i) {
      const Image& m = im[(size_t)i];
      const mpe::GatherFormat f = format_of(m);
      size_t k = 0;
      while (k < fmts.size() && std::memcmp(&fmts[k], &f, sizeof(f))) ++k;
      if (k == fmts.size()) fmts.push_back(f);
      const int s = slot_of[(size_t)i];
      tab[(size_t)s] = mpe::GatherItem{m.img, m.x, m.y, m.w, m.h, s, (int)k};
      item_of_slot[(size_t)s] = i;
      want_slot(m, &want[(size_t)s * slot_bytes], pitch);
    }
    tables += (long)fmts.size();
    const size_t segs_per_slot = (size_t)g_rows * segs_per_row;
    for (size_t idx = 0; idx < (size_t)n * segs_per_slot; ++idx) {  // what k_gather_rois_formats does with segment idx
      const int e = (int)(idx / segs_per_slot);
      const int rem = (int)(idx - (size_t)e * segs_per_slot);
      const int r = rem / segs_per_row, seg = rem - r * segs_per_row;
      const mpe::GatherItem it = tab[(size_t)e];
      const Image& m = im[(size_t)item_of_slot[(size_t)e]];
      const CheckedLoads mem{reinterpret_cast<uintptr_t>(m.img), reinterpret_cast<uintptr_t>(m.img) + m.img_bytes, &dwords,
                             &bytes};
      uint32_t o[4];
      mpe::gather_segment_format(mem, it.img, fmts[(size_t)it.format], it.x, it.y, it.w, it.h, r, seg, o);
      std::memcpy(&got[(size_t)it.slot * slot_bytes + ((size_t)r * segs_per_row + seg) * 16], o, 16);
      ++segments;
    }
    if (got != want) {
      size_t k = 0;
      while (got[k] == want[k]) ++k;
      return report("format table", c, im[(size_t)item_of_slot[k / slot_bytes]], g_rows, pitch, k % slot_bytes, got[k], want[k]);
    }
    items += n;
    for (Image& m : im) std::free(m.buf);
  }
  std::printf("gather_sensor_host ok: formats %d cases, %ld items (rggb %d, bggr %d, gbrg %d, grbg %d, yuv422 %d, yuv422_yuy2 %d, "
              "mono8 %d, bgr8 %d), %ld format table entries, %ld segments, %ld dword loads, %ld byte loads\n", n_cases, items,
              per_enc[0], per_enc[1], per_enc[2], per_enc[3], per_enc[4], per_enc[5], per_enc[6], per_enc[7], tables, segments,
              dwords, bytes);
  return 0;
}
