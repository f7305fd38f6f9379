// mpe_gather.h — one 16-byte segment of a ROI slot, read from an image of arbitrary base, stride and ROI origin: the
// arithmetic of k_gather_rois (mpe_track_device.hip), in a header of its own so that the CPU tier compiles it for the
// host (tests/host/gather_host.cpp) and runs it under AddressSanitizer.
//
// A slot is what pack_roi (mpe_track_abi.cpp) writes on the host: row r < roi_h holds the roi_w bytes of image row
// roi_y + r from column roi_x on, zero up to the pitch; rows from roi_h on are zero.  The source is read as ALIGNED
// dwords that are funnel-shifted into place.  No load touches a byte outside the image [img, img + img_bytes): the
// dword that straddles the first or the last byte of the image is put together from byte loads of the bytes the
// segment wants, and a dword the segment wants nothing of is not loaded.
//
// gather_segment_encoded is the same segment for frames in the camera's own encoding (k_gather_rois_encoded): the 16
// slot bytes are 16 PIXELS of the ROI row, decoded from 2 (mono16), 3 (bgr8 / rgb8) or 4 (bgra8 / rgba8) source bytes
// each by the rules of mpe_pixel.h — the bytes mpe_convert_to_mono8 would have written into a mono8 copy of the frame.
// x, y, w, h stay in pixels; stride and img_bytes are source bytes.
//
// gather_segment_yuv is the 2-byte segment with byte selection in place of mono16_px (yuv422 / yuv422_yuy2).
// gather_segment_bayer is the first NEIGHBOURHOOD decode: the 16 pixels of a slot row come from the 3 x 3 surroundings
// of their (clamped, see bayer_site) sites, three image rows of 18 source bytes, which cross the ROI's edge but never
// the image's.  Both keep every property stated above.
//
// gather_segment_format is the segment of a submission whose items differ in image format (k_gather_rois_formats):
// stride, image end, bytes per pixel and channel / byte order come from the item's entry of a format table, and the
// segment is the one of the functions above that the entry names.  Every property stated above holds per item,
// against the item's OWN image end.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mpe_pixel.h"

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

namespace mpe {

// one slot of a submission (device table, in slot order)
struct GatherItem {
  const uint8_t* img;  // device image of the stream
  int x, y, w, h;      // ROI, inside the image
  int slot;            // destination slot
  int format;          // index into the submission's GatherFormat table (k_gather_rois_formats alone reads it)
};
static_assert(sizeof(GatherItem) == 32, "table entries of 32 bytes");

// one distinct image format of a submission (device table behind the items')
struct GatherFormat {
  uint64_t stride;     // source bytes per row
  uint64_t img_bytes;  // the image ends with the last pixel of its last row: (rows - 1) * stride + cols * bpp
  int bpp;             // source bytes per pixel: 1 mono8 / Bayer, 2 mono16 / YUV, 3 bgr8 / rgb8, 4 bgra8 / rgba8
  int rgb;             // colour pixels are R G B [A] (else B G R [A]); Bayer: the image's cols
  int big_endian;      // the mono16 values are; YUV: the Y byte is byte 1 of the pixel's two; Bayer: the image's rows
  int kind;            // 0 (or PIX_PLAIN): bpp names the decode; PIX_YUV; PIX_BAYER | bayer_phase << 8
};
static_assert(sizeof(GatherFormat) == 32, "table entries of 32 bytes");

// plain loads (on the device from the global address space: global_load instead of flat_load); the host test
// substitutes loads that check their address against the image
#if defined(__HIP_DEVICE_COMPILE__)
#define MPE_GATHER_GLOBAL __attribute__((address_space(1)))
#else
#define MPE_GATHER_GLOBAL
#endif
struct GatherLoads {
  __host__ __device__ uint32_t ld32(uintptr_t a) const { return *reinterpret_cast<const MPE_GATHER_GLOBAL uint32_t*>(a); }
  __host__ __device__ uint32_t ld8(uintptr_t a) const { return *reinterpret_cast<const MPE_GATHER_GLOBAL uint8_t*>(a); }
};

// bytes [16 * seg, 16 * seg + 16) of slot row r -> out[0..3] (little endian).  img_bytes: the image ends with the last
// pixel of its last row, (rows - 1) * stride + cols.
template <class Loads>
__host__ __device__ inline void gather_segment(const Loads& mem, const uint8_t* img, size_t img_bytes, size_t stride, int x,
                                               int y, int w, int h, int r, int seg, uint32_t out[4]) {
  out[0] = out[1] = out[2] = out[3] = 0;
  const int c0 = 16 * seg;
  if (r >= h || c0 >= w) return;
  const int n = w - c0 < 16 ? w - c0 : 16;  // bytes wanted
  const uintptr_t lo = reinterpret_cast<uintptr_t>(img), hi = lo + img_bytes;
  const uintptr_t src = lo + (size_t)(y + r) * stride + (size_t)(x + c0), end = src + (size_t)n;
  const unsigned sh = (unsigned)(src & 3);
  const uintptr_t base = src - sh;  // aligned; up to 3 bytes in front of src (and of the image)
  uint32_t d[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const uintptr_t a = base + 4 * (uintptr_t)j;
    uint32_t v = 0;
    if (a < end) {
      if (a >= lo && a + 4 <= hi) {
        v = mem.ld32(a);
      } else {  // the dword straddles an end of the image: the wanted bytes of it, one by one
        for (int b = 0; b < 4; ++b)
          if (a + b >= src && a + b < end) v |= mem.ld8(a + b) << (8 * b);
      }
    }
    d[j] = v;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // (v_alignbyte_b32 on the device)
    const uint32_t v = (uint32_t)(((((uint64_t)d[i + 1]) << 32) | d[i]) >> (8 * sh));
    const int valid = n - 4 * i;  // bytes of this dword inside the ROI row
    out[i] = valid >= 4 ? v : (valid <= 0 ? 0u : v & ((1u << (8 * valid)) - 1u));
  }
}

// pixels [16 * seg, 16 * seg + 16) of slot row r, decoded from BPP source bytes each -> out[0..3] (little endian).
// img_bytes: the image ends with the last pixel of its last row, (rows - 1) * stride + cols * BPP.  rgb: the colour
// pixels are R G B [A] (else B G R [A]); big_endian: the mono16 values are (BPP 2 alone reads it).  YUV (BPP 2): the
// pixel is the Y byte of its two source bytes, byte 1 when big_endian (yuv422) and byte 0 otherwise (yuv422_yuy2).
template <int BPP, class Loads, bool YUV = false>
__host__ __device__ inline void gather_segment_encoded(const Loads& mem, const uint8_t* img, size_t img_bytes, size_t stride,
                                                       int x, int y, int w, int h, int r, int seg, bool rgb, bool big_endian,
                                                       uint32_t out[4]) {
  static_assert(BPP == 2 || BPP == 3 || BPP == 4, "mono16, bgr8 / rgb8, bgra8 / rgba8");
  out[0] = out[1] = out[2] = out[3] = 0;
  const int c0 = 16 * seg;
  if (r >= h || c0 >= w) return;
  const int n = w - c0 < 16 ? w - c0 : 16;  // pixels wanted
  const uintptr_t lo = reinterpret_cast<uintptr_t>(img), hi = lo + img_bytes;
  const uintptr_t src = lo + (size_t)(y + r) * stride + (size_t)(x + c0) * BPP, end = src + (size_t)n * BPP;
  const unsigned sh = (unsigned)(src & 3);
  const uintptr_t base = src - sh;  // aligned; up to 3 bytes in front of src (and of the image)
  constexpr int ND = 4 * BPP;       // source dwords of 16 pixels
  uint32_t d[ND + 1];
#pragma unroll
  for (int j = 0; j < ND + 1; ++j) {
    const uintptr_t a = base + 4 * (uintptr_t)j;
    uint32_t v = 0;
    if (a < end) {
      if (a >= lo && a + 4 <= hi) {
        v = mem.ld32(a);
      } else {  // the dword straddles an end of the image: the wanted bytes of it, one by one
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (a + b >= src && a + b < end) v |= mem.ld8(a + b) << (8 * b);
      }
    }
    d[j] = v;
  }
  uint32_t s[ND];  // the source bytes from src on
#pragma unroll
  for (int i = 0; i < ND; ++i) s[i] = (uint32_t)(((((uint64_t)d[i + 1]) << 32) | d[i]) >> (8 * sh));
  unsigned px[16];
  if constexpr (BPP == 2 && YUV) {
    const unsigned ysh = big_endian ? 8u : 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      px[2 * k] = (s[k] >> ysh) & 0xFFu;
      px[2 * k + 1] = (s[k] >> (16u + ysh)) & 0xFFu;
    }
  } else if constexpr (BPP == 2) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      unsigned a = s[k] & 0xFFFFu, b = s[k] >> 16;
      if (big_endian) {
        a = ((a & 0xFFu) << 8) | (a >> 8);
        b = ((b & 0xFFu) << 8) | (b >> 8);
      }
      px[2 * k] = mono16_px(a);
      px[2 * k + 1] = mono16_px(b);
    }
  } else if constexpr (BPP == 3) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // four pixels in three dwords
      const uint32_t w0 = s[3 * q], w1 = s[3 * q + 1], w2 = s[3 * q + 2];
      px[4 * q] = gray_px(w0 & 0xFF, (w0 >> 8) & 0xFF, (w0 >> 16) & 0xFF, rgb);
      px[4 * q + 1] = gray_px(w0 >> 24, w1 & 0xFF, (w1 >> 8) & 0xFF, rgb);
      px[4 * q + 2] = gray_px((w1 >> 16) & 0xFF, w1 >> 24, w2 & 0xFF, rgb);
      px[4 * q + 3] = gray_px((w2 >> 8) & 0xFF, (w2 >> 16) & 0xFF, w2 >> 24, rgb);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) px[k] = gray_px(s[k] & 0xFF, (s[k] >> 8) & 0xFF, (s[k] >> 16) & 0xFF, rgb);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (4 * i + b < n) v |= px[4 * i + b] << (8 * b);  // (pixels beyond the ROI row hold whatever lay behind it)
    out[i] = v;
  }
}

// pixels [16 * seg, 16 * seg + 16) of slot row r from a YUV 4:2:2 image: the Y byte of every pixel's two source bytes,
// byte y_byte (yuv_y_byte).  img_bytes = (rows - 1) * stride + cols * 2.
template <class Loads>
__host__ __device__ inline void gather_segment_yuv(const Loads& mem, const uint8_t* img, size_t img_bytes, size_t stride, int x,
                                                   int y, int w, int h, int r, int seg, int y_byte, uint32_t out[4]) {
  gather_segment_encoded<2, Loads, true>(mem, img, img_bytes, stride, x, y, w, h, r, seg, false, y_byte != 0, out);
}

// pixels [16 * seg, 16 * seg + 16) of slot row r from a Bayer image of rows x cols pixels (img_bytes = (rows - 1) *
// stride + cols), decoded by bayer_px.  Output pixel (Y, X) = (y + r, x + c) takes the value of the interior site
// (bayer_site(Y, rows), bayer_site(X, cols)), whose colour comes from its IMAGE coordinates.  The sites of the 16 pixels
// are consecutive columns from cxa = bayer_site(x + 16 * seg, cols) on; their surroundings are the source columns
// cxa - 1 .. cxa + 16 of the image rows cy - 1, cy, cy + 1: three times up to six aligned dwords, of which only those
// are loaded that hold a column the segment needs, all of them inside their image row (1 <= cxa, last site <= cols - 2).
// The values v[j] of the sites cxa + j are then put where the clamp sends them: pixel k is v[k], or v[k - 1] behind
// image column 0 (whose site is column 1), and the image's last column repeats the pixel in front of it.
template <class Loads>
__host__ __device__ inline void gather_segment_bayer(const Loads& mem, const uint8_t* img, size_t img_bytes, size_t stride,
                                                     int rows, int cols, int x, int y, int w, int h, int r, int seg,
                                                     int phase, uint32_t out[4]) {
  out[0] = out[1] = out[2] = out[3] = 0;
  const int c0 = 16 * seg;
  if (r >= h || c0 >= w || rows < 3 || cols < 3) return;  // (an image below 3 x 3 decodes to zeros)
  const int n = w - c0 < 16 ? w - c0 : 16;                // pixels wanted
  const int X0 = x + c0;                                  // image column of pixel 0
  const int cy = bayer_site(y + r, rows), cxa = bayer_site(X0, cols);
  const int cxb = bayer_site(X0 + n - 1, cols);           // the last site: source columns cxa - 1 .. cxb + 1 are wanted
  const uintptr_t lo = reinterpret_cast<uintptr_t>(img), hi = lo + img_bytes;
  uint32_t up[5], mid[5], dn[5];  // 18 source bytes from column cxa - 1 on, of the rows cy - 1, cy, cy + 1
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const uintptr_t src = lo + (size_t)(cy - 1 + q) * stride + (size_t)(cxa - 1), end = src + (size_t)(cxb - cxa + 3);
    const unsigned sh = (unsigned)(src & 3);
    const uintptr_t base = src - sh;  // aligned; up to 3 bytes in front of src (and of the image)
    uint32_t d[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const uintptr_t a = base + 4 * (uintptr_t)j;
      uint32_t v = 0;
      if (a < end) {
        if (a >= lo && a + 4 <= hi) {
          v = mem.ld32(a);
        } else {  // the dword straddles an end of the image: the wanted bytes of it, one by one
#pragma unroll
          for (int b = 0; b < 4; ++b)
            if (a + b >= src && a + b < end) v |= mem.ld8(a + b) << (8 * b);
        }
      }
      d[j] = v;
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const uint32_t v = (uint32_t)(((((uint64_t)d[i + 1]) << 32) | d[i]) >> (8 * sh));
      if (q == 0) up[i] = v;
      else if (q == 1) mid[i] = v;
      else dn[i] = v;
    }
  }
  unsigned vs[18], ms[18];  // per source column: up + down, and the middle row
#pragma unroll
  for (int i = 0; i < 18; ++i) {
    const unsigned b = 8u * (unsigned)(i & 3);
    vs[i] = ((up[i >> 2] >> b) & 0xFFu) + ((dn[i >> 2] >> b) & 0xFFu);
    ms[i] = (mid[i >> 2] >> b) & 0xFFu;
  }
  unsigned v[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = bayer_px(vs[j] + vs[j + 2], vs[j + 1], ms[j] + ms[j + 2], ms[j + 1], cy, cxa + j, phase);
  unsigned px[16];
  const bool left = X0 == 0;       // pixel 0 is image column 0: pixels 0 and 1 share the site of column 1
  const int kr = cols - 1 - X0;    // the pixel that is the image's last column (if 1 .. 15: it repeats pixel kr - 1)
  px[0] = v[0];
#pragma unroll
  for (int k = 1; k < 16; ++k) px[k] = left ? v[k - 1] : v[k];
#pragma unroll
  for (int k = 1; k < 16; ++k)
    if (k == kr) px[k] = px[k - 1];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t o = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (4 * i + b < n) o |= px[4 * i + b] << (8 * b);  // (pixels beyond the ROI row were computed from zeros)
    out[i] = o;
  }
}

// the same 16 slot bytes from an image of format f: the segment function f names.  SENSOR false: for tables that hold no
// YUV or Bayer entry (the kernel of such a submission is then the one it was before those existed)
template <bool SENSOR = true, class Loads>
__host__ __device__ inline void gather_segment_format(const Loads& mem, const uint8_t* img, const GatherFormat& f, int x, int y,
                                                      int w, int h, int r, int seg, uint32_t out[4]) {
  const size_t stride = (size_t)f.stride, img_bytes = (size_t)f.img_bytes;
  if constexpr (SENSOR) {
    if ((f.kind & 0xFF) == PIX_YUV) {
      gather_segment_yuv(mem, img, img_bytes, stride, x, y, w, h, r, seg, f.big_endian, out);
      return;
    }
    if ((f.kind & 0xFF) == PIX_BAYER) {
      gather_segment_bayer(mem, img, img_bytes, stride, f.big_endian, f.rgb, x, y, w, h, r, seg, f.kind >> 8, out);
      return;
    }
  }
  switch (f.bpp) {
    case 1:
      gather_segment(mem, img, img_bytes, stride, x, y, w, h, r, seg, out);
      break;
    case 2:
      gather_segment_encoded<2>(mem, img, img_bytes, stride, x, y, w, h, r, seg, false, f.big_endian != 0, out);
      break;
    case 3:
      gather_segment_encoded<3>(mem, img, img_bytes, stride, x, y, w, h, r, seg, f.rgb != 0, false, out);
      break;
    default:
      gather_segment_encoded<4>(mem, img, img_bytes, stride, x, y, w, h, r, seg, f.rgb != 0, false, out);
      break;
  }
}

}  // namespace mpe
