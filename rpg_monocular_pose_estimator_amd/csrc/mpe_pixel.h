// mpe_pixel.h — one source pixel of a sensor_msgs/Image payload -> mono8: what cv_bridge::toCvCopy(msg, MONO8) does for
// the node (monocular_pose_estimator.cpp:147), defined ONCE for k_to_mono8 (mpe_k3.hip, the whole-frame decode),
// k_gather_rois_encoded (mpe_track_device.hip through mpe_gather.h, the decode inside the ROI gather) and the host tier.
//   bgr8 / rgb8 / bgra8 / rgba8: cv::cvtColor(..., COLOR_*2GRAY) for CV_8U — integer, 14 fractional bits,
//       Y = (B * 1868 + G * 9617 + R * 4899 + 2^13) >> 14   (OpenCV 2.4, 3.0 .. 3.4.1; from 3.4.2 on: 15 bits, see mpe.h)
//   mono16 (host byte order after cv_bridge's endianness fix): Mat::convertTo(CV_8U, 255. / 65535.) —
//       saturate_cast<uchar>((float)v * (float)(255. / 65535.)), i.e. round-half-even of the single-precision product
//   yuv422 (U Y V Y) / yuv422_yuy2 (Y U Y V): COLOR_YUV2GRAY_UYVY / _YUY2 — the pixel's Y byte, byte 1 / byte 0 of its
//       two source bytes (yuv_y_byte), an exact copy
//   bayer_rggb8 / bggr8 / gbrg8 / grbg8: COLOR_Bayer*2GRAY, OpenCV's scalar Bayer2Gray (bayer_px): the 3 x 3 surroundings
//       of an INTERIOR pixel, every neighbour weighted by the 14-bit weight of its own colour; the border rows and
//       columns repeat their inner neighbours (bayer_site) and an image below 3 x 3 is all zeros.  Unpinned: see mpe.h
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/mpe.h"

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

namespace mpe {

// c0, c1, c2: the first three bytes of the pixel in memory order (B G R, or R G B when rgb)
__host__ __device__ inline unsigned gray_px(unsigned c0, unsigned c1, unsigned c2, bool rgb) {
  const unsigned b = rgb ? c2 : c0, r = rgb ? c0 : c2;
  return (b * 1868u + c1 * 9617u + r * 4899u + (1u << 13)) >> 14;
}

// v: the 16-bit value in host byte order
__host__ __device__ inline unsigned mono16_px(unsigned v) {
  float r = rintf((float)v * (float)(255.0 / 65535.0));
  r = fminf(fmaxf(r, 0.f), 255.f);
  return (unsigned)r;
}

// what decodes a pixel.  Bytes per pixel do not say it: Bayer shares 1 with mono8, YUV shares 2 with mono16
enum PixelKind { PIX_NONE = 0, PIX_PLAIN = 1, PIX_YUV = 2, PIX_BAYER = 3 };  // PLAIN: mono8, colour, mono16
__host__ __device__ inline int encoding_kind(int encoding) {
  if (encoding >= MPE_ENC_MONO8 && encoding <= MPE_ENC_MONO16) return PIX_PLAIN;
  if (encoding >= MPE_ENC_BAYER_RGGB8 && encoding <= MPE_ENC_BAYER_GRBG8) return PIX_BAYER;
  if (encoding == MPE_ENC_YUV422 || encoding == MPE_ENC_YUV422_YUY2) return PIX_YUV;
  return PIX_NONE;
}

// source bytes per pixel of an MPE_ENC_* encoding, 0 for anything else (MPE_ERR_UNSUPPORTED)
__host__ __device__ inline int encoding_bytes_per_pixel(int encoding) {
  switch (encoding) {
    case MPE_ENC_MONO8: return 1;
    case MPE_ENC_MONO16: return 2;
    case MPE_ENC_BGR8: case MPE_ENC_RGB8: return 3;
    case MPE_ENC_BGRA8: case MPE_ENC_RGBA8: return 4;
    case MPE_ENC_BAYER_RGGB8: case MPE_ENC_BAYER_BGGR8: case MPE_ENC_BAYER_GBRG8: case MPE_ENC_BAYER_GRBG8: return 1;
    case MPE_ENC_YUV422: case MPE_ENC_YUV422_YUY2: return 2;
    default: return 0;
  }
}

// ---- an image format (mpe_image_format: rows, cols, stride in source bytes, encoding, byte order) on the host: what the
// tracked entries ask of one, stated once for mpe_track_abi.cpp and mpe_tracker.cpp.  No handle, no HIP call.

// the bytes from an image's first pixel to the last pixel of its last row (rows >= 1, a known encoding): what a device
// allocation must hold of it, and where the gathers stop reading
inline size_t image_extent(const mpe_image_format& f) {
  return (size_t)(f.rows - 1) * f.stride_bytes + (size_t)f.cols * (size_t)encoding_bytes_per_pixel(f.encoding);
}

// two formats name the same images: size, stride, encoding and — for mono16, which alone reads it — the byte order
inline bool same_image_format(const mpe_image_format& a, const mpe_image_format& b) {
  return a.rows == b.rows && a.cols == b.cols && a.stride_bytes == b.stride_bytes && a.encoding == b.encoding &&
         (a.encoding != MPE_ENC_MONO16 || (a.src_big_endian != 0) == (b.src_big_endian != 0));
}

// Why images of a format are refused: the code and the text for mpe_last_error, or {MPE_OK, null}.  Three rules, each
// stated once; an entry asks them in order and the first that fails answers.
struct FormatRefusal {
  int code;
  const char* msg;
};
// the encoding is one the library knows and can decode from where the frames are
inline FormatRefusal refuse_encoding(int encoding, bool on_device) {
  if (!encoding_bytes_per_pixel(encoding)) return {MPE_ERR_UNSUPPORTED, "encoding not supported (one of MPE_ENC_*)"};
  if (!on_device && encoding_kind(encoding) != PIX_PLAIN)  // (what these codes answered before they existed)
    return {MPE_ERR_UNSUPPORTED, "encoding not supported for host frames (Bayer and YUV: device frames)"};
  return {MPE_OK, nullptr};
}
// host frames are packed, not decoded (a rule for formats that have images in the call)
inline FormatRefusal refuse_host_encoding(int encoding, bool on_device) {
  if (!on_device && encoding != MPE_ENC_MONO8)
    return {MPE_ERR_ARG, "host frames are mono8 (the encodings are decoded from device frames)"};
  return {MPE_OK, nullptr};
}
// a size, and a stride that holds a row (of a known encoding)
inline FormatRefusal refuse_size(const mpe_image_format& f) {
  if (f.rows < 1 || f.cols < 1 || f.stride_bytes < (size_t)f.cols * (size_t)encoding_bytes_per_pixel(f.encoding))
    return {MPE_ERR_ARG, "bad argument"};
  return {MPE_OK, nullptr};
}
// The two orders the entries ask them in.  check_format_shape: the format as such, with or without images in the call —
// encoding, then size.  check_image_format: a format that has images — the same, then the host rule.
// (mpe_track_step_batch_wide alone asks the host rule before the size: mpe_track_abi.cpp.)
inline FormatRefusal check_format_shape(const mpe_image_format& f, bool on_device) {
  const FormatRefusal r = refuse_encoding(f.encoding, on_device);
  return r.code != MPE_OK ? r : refuse_size(f);
}
inline FormatRefusal check_image_format(const mpe_image_format& f, bool on_device) {
  const FormatRefusal r = check_format_shape(f, on_device);
  return r.code != MPE_OK ? r : refuse_host_encoding(f.encoding, on_device);
}

// which of a YUV 4:2:2 pixel's two source bytes is its Y: 1 for yuv422 (U Y V Y), 0 for yuv422_yuy2 (Y U Y V)
__host__ __device__ inline int yuv_y_byte(int encoding) { return encoding == MPE_ENC_YUV422 ? 1 : 0; }

// Bayer phase: the parities of the rows (bit 1) and columns (bit 0) that hold the RED sites; blue sits on the other
// parity of both, green on the rest.  rggb 0, grbg 1, gbrg 2, bggr 3
__host__ __device__ inline int bayer_phase(int encoding) {
  switch (encoding) {
    case MPE_ENC_BAYER_GRBG8: return 1;
    case MPE_ENC_BAYER_GBRG8: return 2;
    case MPE_ENC_BAYER_BGGR8: return 3;
    default: return 0;
  }
}

// the interior site whose value output pixel v (a row or a column index) of n takes; n >= 3
__host__ __device__ inline int bayer_site(int v, int n) { return v < 1 ? 1 : (v > n - 2 ? n - 2 : v); }

// One interior site (y, x) — IMAGE coordinates, they give the colour — from the sums over its 3 x 3 surroundings:
// diag = the four diagonal neighbours, vert = up + down, horiz = left + right, c = the centre.
__host__ __device__ inline unsigned bayer_px(unsigned diag, unsigned vert, unsigned horiz, unsigned c, int y, int x,
                                             int phase) {
  const bool red_row = (y & 1) == (phase >> 1), red_col = (x & 1) == (phase & 1);
  if (red_row == red_col) {  // a red or a blue site: the diagonals have the other colour, the edges are green
    const unsigned wx = red_row ? 4899u : 1868u, wz = red_row ? 1868u : 4899u;
    return (wz * diag + 9617u * (vert + horiz) + 4u * wx * c + (1u << 15)) >> 16;
  }
  // a green site: red left and right in a red row (blue above and below), the other way round in a blue row
  const unsigned wh = red_row ? 4899u : 1868u, wv = red_row ? 1868u : 4899u;
  return (wv * vert + wh * horiz + 2u * 9617u * c + (1u << 14)) >> 15;
}

}  // namespace mpe
