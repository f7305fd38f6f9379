// image_format_host.cpp — what the tracked entries ask of an image format (csrc/mpe_pixel.h: the three rules
// refuse_encoding, refuse_host_encoding, refuse_size; check_format_shape and check_image_format, the two orders they
// are asked in; image_extent, same_image_format), as a stand-alone host program that
// tests/test_image_format_checks.py builds with -fsanitize=address,undefined and runs.  These functions need no handle and
// no device, so the table of refusals that is otherwise seen only through a handle's mpe_last_error is pinned here:
//   every MPE_ENC_* code and one code outside them (6), for host and for device frames: the code and the text;
//   the size and stride edges: rows = 0, cols = 0, stride = cols * bpp - 1 refused, stride = cols * bpp accepted;
//   which refusal answers when two rules fail (the encoding before the size, the size before "host frames are mono8");
//   the order of mpe_track_step_batch_wide alone: "host frames are mono8" before the size;
//   image_extent for one image per bytes-per-pixel value, a single row, and an extent beyond 2^32;
//   same_image_format: every field counts, the byte order for mono16 alone.
#include <cstdio>
#include <cstring>

#include "mpe_pixel.h"

namespace {

const char* const kUnknown = "encoding not supported (one of MPE_ENC_*)";
const char* const kHostSensor = "encoding not supported for host frames (Bayer and YUV: device frames)";
const char* const kHostMono8 = "host frames are mono8 (the encodings are decoded from device frames)";
const char* const kBad = "bad argument";

int failures = 0;

void expect(const char* what, const mpe_image_format& f, bool on_device, mpe::FormatRefusal got, int code, const char* msg) {
  const bool same_msg = (!got.msg && !msg) || (got.msg && msg && !std::strcmp(got.msg, msg));
  if (got.code == code && same_msg) return;
  std::fprintf(stderr, "%s: %d x %d stride %zu encoding %d on_device %d: (%d, %s), expected (%d, %s)\n", what, f.rows, f.cols,
               f.stride_bytes, f.encoding, (int)on_device, got.code, got.msg ? got.msg : "null", code, msg ? msg : "null");
  ++failures;
}

// both checks; `shape_*` where the format as such answers differently from the format with images in the call
void expect_both(const mpe_image_format& f, bool on_device, int code, const char* msg, int shape_code, const char* shape_msg) {
  expect("check_image_format", f, on_device, mpe::check_image_format(f, on_device), code, msg);
  expect("check_format_shape", f, on_device, mpe::check_format_shape(f, on_device), shape_code, shape_msg);
}
void expect_both(const mpe_image_format& f, bool on_device, int code, const char* msg) {
  expect_both(f, on_device, code, msg, code, msg);
}

struct Enc {
  int code, bpp;
  bool plain;
};
const Enc kEncodings[12] = {{MPE_ENC_MONO8, 1, true},         {MPE_ENC_BGR8, 3, true},          {MPE_ENC_RGB8, 3, true},
                            {MPE_ENC_BGRA8, 4, true},         {MPE_ENC_RGBA8, 4, true},         {MPE_ENC_MONO16, 2, true},
                            {MPE_ENC_BAYER_RGGB8, 1, false},  {MPE_ENC_BAYER_BGGR8, 1, false},  {MPE_ENC_BAYER_GBRG8, 1, false},
                            {MPE_ENC_BAYER_GRBG8, 1, false},  {MPE_ENC_YUV422, 2, false},       {MPE_ENC_YUV422_YUY2, 2, false}};

void expect_extent(const mpe_image_format& f, size_t want) {
  if (mpe::image_extent(f) == want) return;
  std::fprintf(stderr, "image_extent: %d x %d stride %zu encoding %d: %zu, expected %zu\n", f.rows, f.cols, f.stride_bytes,
               f.encoding, mpe::image_extent(f), want);
  ++failures;
}

void expect_same(const mpe_image_format& a, const mpe_image_format& b, bool want, const char* what) {
  if (mpe::same_image_format(a, b) == want && mpe::same_image_format(b, a) == want) return;
  std::fprintf(stderr, "same_image_format (%s): expected %d\n", what, (int)want);
  ++failures;
}

}  // namespace

int main() {
  // ---- every encoding, a good size (48 x 64, rows 8 bytes longer than they must be)
  for (const Enc& e : kEncodings) {
    const mpe_image_format f = {48, 64, (size_t)64 * e.bpp + 8, e.code, 0};
    expect_both(f, true, MPE_OK, nullptr);
    if (e.code == MPE_ENC_MONO8)
      expect_both(f, false, MPE_OK, nullptr);
    else if (e.plain)  // (decodable, so the format as such is good; only with host images in the call it is refused)
      expect_both(f, false, MPE_ERR_ARG, kHostMono8, MPE_OK, nullptr);
    else
      expect_both(f, false, MPE_ERR_UNSUPPORTED, kHostSensor);
  }
  const int unknown[4] = {6, 15, 22, -1};  // outside MPE_ENC_*
  for (int code : unknown) {
    const mpe_image_format f = {48, 64, 256, code, 0};
    expect_both(f, true, MPE_ERR_UNSUPPORTED, kUnknown);
    expect_both(f, false, MPE_ERR_UNSUPPORTED, kUnknown);
  }
  // ---- the size and stride edges, per encoding on the device and for mono8 on the host
  for (const Enc& e : kEncodings)
    for (int on_device = 0; on_device < 2; ++on_device) {
      if (!on_device && e.code != MPE_ENC_MONO8) continue;
      const size_t row = (size_t)64 * e.bpp;
      expect_both(mpe_image_format{0, 64, row, e.code, 0}, on_device != 0, MPE_ERR_ARG, kBad);
      expect_both(mpe_image_format{-1, 64, row, e.code, 0}, on_device != 0, MPE_ERR_ARG, kBad);
      expect_both(mpe_image_format{48, 0, row, e.code, 0}, on_device != 0, MPE_ERR_ARG, kBad);
      expect_both(mpe_image_format{48, 64, row - 1, e.code, 0}, on_device != 0, MPE_ERR_ARG, kBad);
      expect_both(mpe_image_format{48, 64, row, e.code, 0}, on_device != 0, MPE_OK, nullptr);
      expect_both(mpe_image_format{1, 1, (size_t)e.bpp, e.code, 0}, on_device != 0, MPE_OK, nullptr);
    }
  // ---- two rules fail: the first one answers
  expect_both(mpe_image_format{0, 0, 0, 6, 0}, true, MPE_ERR_UNSUPPORTED, kUnknown);                   // encoding, then size
  expect_both(mpe_image_format{0, 64, 64, MPE_ENC_YUV422, 0}, false, MPE_ERR_UNSUPPORTED, kHostSensor);  // ... on the host too
  expect_both(mpe_image_format{48, 64, 3 * 64 - 1, MPE_ENC_BGR8, 0}, false, MPE_ERR_ARG, kBad);        // size, then host mono8
  expect_both(mpe_image_format{0, 64, 128, MPE_ENC_MONO16, 1}, false, MPE_ERR_ARG, kBad);
  // ---- the wide entry's order (its own rows / cols condition comes first): encoding, host rule, size
  {
    const mpe_image_format f = {48, 64, 3 * 64 - 1, MPE_ENC_BGR8, 0};  // host bgr8 with a short stride
    mpe::FormatRefusal no = mpe::refuse_encoding(f.encoding, false);
    if (no.code == MPE_OK) no = mpe::refuse_host_encoding(f.encoding, false);
    if (no.code == MPE_OK) no = mpe::refuse_size(f);
    expect("wide order", f, false, no, MPE_ERR_ARG, kHostMono8);
    expect("refuse_size", f, false, mpe::refuse_size(f), MPE_ERR_ARG, kBad);
    expect("refuse_host_encoding", f, true, mpe::refuse_host_encoding(f.encoding, true), MPE_OK, nullptr);
    expect("refuse_encoding", f, false, mpe::refuse_encoding(MPE_ENC_BAYER_GRBG8, false), MPE_ERR_UNSUPPORTED, kHostSensor);
    expect("refuse_encoding", f, true, mpe::refuse_encoding(MPE_ENC_BAYER_GRBG8, true), MPE_OK, nullptr);
  }
  // ---- image_extent: to the last pixel of the last row, in source bytes
  expect_extent(mpe_image_format{3, 5, 8, MPE_ENC_MONO8, 0}, 21);
  expect_extent(mpe_image_format{4, 7, 20, MPE_ENC_MONO16, 0}, 74);
  expect_extent(mpe_image_format{2, 5, 16, MPE_ENC_BGR8, 0}, 31);
  expect_extent(mpe_image_format{3, 2, 8, MPE_ENC_RGBA8, 0}, 24);
  expect_extent(mpe_image_format{3, 5, 8, MPE_ENC_BAYER_GBRG8, 0}, 21);
  expect_extent(mpe_image_format{4, 7, 20, MPE_ENC_YUV422, 0}, 74);
  for (const Enc& e : kEncodings)  // one row: the stride does not enter
    expect_extent(mpe_image_format{1, 9, 4096, e.code, 0}, (size_t)9 * e.bpp);
  expect_extent(mpe_image_format{1200, 1920, 1936, MPE_ENC_MONO8, 0}, 2323184);
  expect_extent(mpe_image_format{70000, 70000, 70000, MPE_ENC_MONO8, 0}, (size_t)4900000000ull);  // (no 32-bit product)
  // ---- same_image_format
  const mpe_image_format a = {480, 752, 760, MPE_ENC_BGR8, 0};
  expect_same(a, a, true, "itself");
  expect_same(a, mpe_image_format{481, 752, 760, MPE_ENC_BGR8, 0}, false, "rows");
  expect_same(a, mpe_image_format{480, 751, 760, MPE_ENC_BGR8, 0}, false, "cols");
  expect_same(a, mpe_image_format{480, 752, 768, MPE_ENC_BGR8, 0}, false, "stride");
  expect_same(a, mpe_image_format{480, 752, 760, MPE_ENC_RGB8, 0}, false, "encoding");
  expect_same(a, mpe_image_format{480, 752, 760, MPE_ENC_BGR8, 1}, true, "byte order of bgr8 is not read");
  const mpe_image_format m = {480, 752, 1504, MPE_ENC_MONO16, 0};
  expect_same(m, mpe_image_format{480, 752, 1504, MPE_ENC_MONO16, 1}, false, "byte order of mono16");
  expect_same(mpe_image_format{480, 752, 1504, MPE_ENC_MONO16, 2}, mpe_image_format{480, 752, 1504, MPE_ENC_MONO16, 1}, true,
              "any non-zero byte order is big-endian");
  expect_same(mpe_image_format{480, 752, 1504, MPE_ENC_YUV422, 0}, mpe_image_format{480, 752, 1504, MPE_ENC_YUV422, 1}, true,
              "byte order of yuv422 is not read");
  if (failures) return 1;
  std::printf("image_format_host ok: 12 encodings + 4 unknown codes, host and device; edges; precedence; extents; equality\n");
  return 0;
}
