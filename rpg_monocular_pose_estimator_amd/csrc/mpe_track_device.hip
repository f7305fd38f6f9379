// mpe_track_device.hip — the ROI gather of lock-step submissions whose frames are in DEVICE memory
// (mpe_track_step_batch_setups_device[_submit]): submit_slots (mpe_track_abi.cpp) does not pack the ROI slots on the
// host and copy them, k_gather_rois writes them from the caller's device images.  The slot bytes are those pack_roi
// writes, so everything behind them is the host-frame submission's.  k_gather_rois_encoded does the same for frames in
// the camera's own encoding (mpe_track_step_batch_setups_device_encoded[_submit]): it decodes the pixels it gathers, so
// no mono8 copy of the frames is made first.  k_gather_rois_formats serves a submission whose items differ in image
// format (mpe_track_step_batch_formats[_submit]): stride, image end and encoding per item, from a format table.
#include "mpe_host.h"
#include "mpe_gather.h"

namespace {

// One thread per 16-byte segment of every slot: aligned dword loads (consecutive lanes read consecutive dwords of an
// image row), one 16-byte store.  Traffic = the slot bytes; at 64 streams of ~120 x 120 that is 1 MB — a launch bound by
// latency, not by bandwidth.
__global__ __launch_bounds__(256) void k_gather_rois(const GatherItem* __restrict__ tab, int n, uint8_t* __restrict__ dst,
                                                     size_t slot_bytes, int rows, int segs_per_row, size_t stride,
                                                     size_t img_bytes) {
  const size_t segs_per_slot = (size_t)rows * segs_per_row;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)n * segs_per_slot) return;
  const int e = (int)(idx / segs_per_slot);
  const int rem = (int)(idx - (size_t)e * segs_per_slot);
  const int r = rem / segs_per_row, seg = rem - r * segs_per_row;
  const GatherItem it = tab[e];
  uint32_t o[4];
  gather_segment(GatherLoads(), it.img, img_bytes, stride, it.x, it.y, it.w, it.h, r, seg, o);
  // (slot base, pitch and segment offset are multiples of 16)
  *reinterpret_cast<uint4*>(dst + (size_t)it.slot * slot_bytes + ((size_t)r * segs_per_row + seg) * 16) =
      make_uint4(o[0], o[1], o[2], o[3]);
}

// The same slots from ENCODED images (BPP source bytes per pixel: 2 mono16, 3 bgr8 / rgb8, 4 bgra8 / rgba8): one thread
// per 16 pixels of a slot row = 16 * BPP source bytes as aligned dwords (consecutive lanes read consecutive runs of an
// image row), decoded by the rules of mpe_pixel.h, one 16-byte store.  The dword array of a segment (4 * BPP + 1) is
// indexed by unrolled loops alone and stays in registers.
template <int BPP>
__global__ __launch_bounds__(256) void k_gather_rois_encoded(const GatherItem* __restrict__ tab, int n,
                                                             uint8_t* __restrict__ dst, size_t slot_bytes, int rows,
                                                             int segs_per_row, size_t stride, size_t img_bytes, int rgb,
                                                             int big_endian) {
  const size_t segs_per_slot = (size_t)rows * segs_per_row;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)n * segs_per_slot) return;
  const int e = (int)(idx / segs_per_slot);
  const int rem = (int)(idx - (size_t)e * segs_per_slot);
  const int r = rem / segs_per_row, seg = rem - r * segs_per_row;
  const GatherItem it = tab[e];
  uint32_t o[4];
  gather_segment_encoded<BPP>(GatherLoads(), it.img, img_bytes, stride, it.x, it.y, it.w, it.h, r, seg, rgb != 0,
                              big_endian != 0, o);
  // (slot base, pitch and segment offset are multiples of 16)
  *reinterpret_cast<uint4*>(dst + (size_t)it.slot * slot_bytes + ((size_t)r * segs_per_row + seg) * 16) =
      make_uint4(o[0], o[1], o[2], o[3]);
}

// The same slots from YUV 4:2:2 images (yuv422 / yuv422_yuy2): the two-byte segment with the Y byte picked out of every
// pixel's pair (gather_segment_yuv); 32 source bytes as aligned dwords, one 16-byte store.
__global__ __launch_bounds__(256) void k_gather_rois_yuv(const GatherItem* __restrict__ tab, int n, uint8_t* __restrict__ dst,
                                                         size_t slot_bytes, int rows, int segs_per_row, size_t stride,
                                                         size_t img_bytes, int y_byte) {
  const size_t segs_per_slot = (size_t)rows * segs_per_row;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)n * segs_per_slot) return;
  const int e = (int)(idx / segs_per_slot);
  const int rem = (int)(idx - (size_t)e * segs_per_slot);
  const int r = rem / segs_per_row, seg = rem - r * segs_per_row;
  const GatherItem it = tab[e];
  uint32_t o[4];
  gather_segment_yuv(GatherLoads(), it.img, img_bytes, stride, it.x, it.y, it.w, it.h, r, seg, y_byte, o);
  // (slot base, pitch and segment offset are multiples of 16)
  *reinterpret_cast<uint4*>(dst + (size_t)it.slot * slot_bytes + ((size_t)r * segs_per_row + seg) * 16) =
      make_uint4(o[0], o[1], o[2], o[3]);
}

// The same slots from BAYER images of img_rows x img_cols pixels: one thread per 16 pixels of a slot row, which come from
// the 3 x 3 surroundings of their sites — 18 source bytes of three image rows as up to 6 aligned dwords each
// (gather_segment_bayer; the rows of a ROI are read three times, from L2 after the first), one 16-byte store.  Every
// dword array is indexed by unrolled loops alone and stays in registers.
__global__ __launch_bounds__(256) void k_gather_rois_bayer(const GatherItem* __restrict__ tab, int n,
                                                           uint8_t* __restrict__ dst, size_t slot_bytes, int rows,
                                                           int segs_per_row, size_t stride, size_t img_bytes, int img_rows,
                                                           int img_cols, int phase) {
  const size_t segs_per_slot = (size_t)rows * segs_per_row;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)n * segs_per_slot) return;
  const int e = (int)(idx / segs_per_slot);
  const int rem = (int)(idx - (size_t)e * segs_per_slot);
  const int r = rem / segs_per_row, seg = rem - r * segs_per_row;
  const GatherItem it = tab[e];
  uint32_t o[4];
  gather_segment_bayer(GatherLoads(), it.img, img_bytes, stride, img_rows, img_cols, it.x, it.y, it.w, it.h, r, seg, phase, o);
  // (slot base, pitch and segment offset are multiples of 16)
  *reinterpret_cast<uint4*>(dst + (size_t)it.slot * slot_bytes + ((size_t)r * segs_per_row + seg) * 16) =
      make_uint4(o[0], o[1], o[2], o[3]);
}

// The same slots from images that differ in FORMAT: item e is an image of fmts[tab[e].format] (stride, image end, bytes
// per pixel, channel / byte order), the segment is the one of the two kernels above for that format
// (gather_segment_format) or, for a YUV or a Bayer entry, of the two kernels in front of this one.  Segments are indexed
// slot after slot, so a wave (64 consecutive segments) holds two slots — and so, at most, two formats — only where one
// slot ends inside it; the submission places the slots of one format next to each other within every set-up range, so
// the branch on the format diverges in those boundary waves alone.  SENSOR: the table may hold YUV and Bayer entries;
// a table without them runs the instantiation without those branches (49 VGPRs instead of 122).
template <bool SENSOR>
__global__ __launch_bounds__(256) void k_gather_rois_formats(const GatherItem* __restrict__ tab,
                                                             const GatherFormat* __restrict__ fmts, int n,
                                                             uint8_t* __restrict__ dst, size_t slot_bytes, int rows,
                                                             int segs_per_row) {
  const size_t segs_per_slot = (size_t)rows * segs_per_row;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)n * segs_per_slot) return;
  const int e = (int)(idx / segs_per_slot);
  const int rem = (int)(idx - (size_t)e * segs_per_slot);
  const int r = rem / segs_per_row, seg = rem - r * segs_per_row;
  const GatherItem it = tab[e];
  const GatherFormat f = fmts[it.format];
  uint32_t o[4];
  gather_segment_format<SENSOR>(GatherLoads(), it.img, f, it.x, it.y, it.w, it.h, r, seg, o);
  // (slot base, pitch and segment offset are multiples of 16)
  *reinterpret_cast<uint4*>(dst + (size_t)it.slot * slot_bytes + ((size_t)r * segs_per_row + seg) * 16) =
      make_uint4(o[0], o[1], o[2], o[3]);
}

}  // namespace

namespace mpe_host {

hipError_t launch_gather_rois(const GatherItem* tab, int n, uint8_t* dst, const FrameGeom& g, size_t stride, size_t img_bytes,
                              hipStream_t s) {
  const size_t total = (size_t)n * g.rows * g.segs_per_row;
  const size_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gather_rois, dim3((unsigned)blocks), dim3(256), 0, s, tab, n, dst, (size_t)g.rows * g.pitch, g.rows,
                     g.segs_per_row, stride, img_bytes);
  return hipGetLastError();
}

hipError_t launch_gather_rois_encoded(const GatherItem* tab, int n, uint8_t* dst, const FrameGeom& g, size_t stride,
                                      size_t img_bytes, int encoding, int big_endian, hipStream_t s) {
  const size_t total = (size_t)n * g.rows * g.segs_per_row;
  const size_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  const int rgb = encoding == MPE_ENC_RGB8 || encoding == MPE_ENC_RGBA8;
  const dim3 grid((unsigned)blocks), block(256);
  const size_t slot_bytes = (size_t)g.rows * g.pitch;
  if (encoding_kind(encoding) == PIX_YUV) {
    hipLaunchKernelGGL(k_gather_rois_yuv, grid, block, 0, s, tab, n, dst, slot_bytes, g.rows, g.segs_per_row, stride, img_bytes,
                       yuv_y_byte(encoding));
    return hipGetLastError();
  }
  if (encoding_kind(encoding) == PIX_BAYER) {
    // the image's size back from its end: img_bytes = (rows - 1) * stride + cols with 1 <= cols <= stride
    if (!stride || !img_bytes) return hipErrorInvalidValue;
    const size_t rows_m1 = (img_bytes - 1) / stride, cols = img_bytes - rows_m1 * stride;
    if (rows_m1 >= 0x7fffffffu || cols > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gather_rois_bayer, grid, block, 0, s, tab, n, dst, slot_bytes, g.rows, g.segs_per_row, stride,
                       img_bytes, (int)rows_m1 + 1, (int)cols, bayer_phase(encoding));
    return hipGetLastError();
  }
  switch (encoding_bytes_per_pixel(encoding)) {
    case 2:
      hipLaunchKernelGGL(k_gather_rois_encoded<2>, grid, block, 0, s, tab, n, dst, slot_bytes, g.rows, g.segs_per_row, stride,
                         img_bytes, 0, big_endian);
      break;
    case 3:
      hipLaunchKernelGGL(k_gather_rois_encoded<3>, grid, block, 0, s, tab, n, dst, slot_bytes, g.rows, g.segs_per_row, stride,
                         img_bytes, rgb, 0);
      break;
    case 4:
      hipLaunchKernelGGL(k_gather_rois_encoded<4>, grid, block, 0, s, tab, n, dst, slot_bytes, g.rows, g.segs_per_row, stride,
                         img_bytes, rgb, 0);
      break;
    default:  // (mono8 goes through launch_gather_rois; anything else was refused by the entry)
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_gather_rois_formats(const GatherItem* tab, const GatherFormat* fmts, int n, uint8_t* dst, const FrameGeom& g,
                                      bool sensor, hipStream_t s) {
  const size_t total = (size_t)n * g.rows * g.segs_per_row;
  const size_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  if (sensor)
    hipLaunchKernelGGL(k_gather_rois_formats<true>, dim3((unsigned)blocks), dim3(256), 0, s, tab, fmts, n, dst,
                       (size_t)g.rows * g.pitch, g.rows, g.segs_per_row);
  else
    hipLaunchKernelGGL(k_gather_rois_formats<false>, dim3((unsigned)blocks), dim3(256), 0, s, tab, fmts, n, dst,
                       (size_t)g.rows * g.pitch, g.rows, g.segs_per_row);
  return hipGetLastError();
}

}  // namespace mpe_host
