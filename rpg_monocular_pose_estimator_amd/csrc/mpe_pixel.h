// mpe_pixel.h — one source pixel of a sensor_msgs/Image payload -> mono8: what cv_bridge::toCvCopy(msg, MONO8) does for
// the node (monocular_pose_estimator.cpp:147), defined ONCE for k_to_mono8 (mpe_k3.hip, the whole-frame decode),
// k_gather_rois_encoded (mpe_track_device.hip through mpe_gather.h, the decode inside the ROI gather) and the host tier.
//   bgr8 / rgb8 / bgra8 / rgba8: cv::cvtColor(..., COLOR_*2GRAY) for CV_8U — integer, 14 fractional bits,
//       Y = (B * 1868 + G * 9617 + R * 4899 + 2^13) >> 14   (OpenCV 2.4, 3.0 .. 3.4.1; from 3.4.2 on: 15 bits, see mpe.h)
//   mono16 (host byte order after cv_bridge's endianness fix): Mat::convertTo(CV_8U, 255. / 65535.) —
//       saturate_cast<uchar>((float)v * (float)(255. / 65535.)), i.e. round-half-even of the single-precision product
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

// source bytes per pixel of an MPE_ENC_* encoding, 0 for anything else (Bayer, YUV: MPE_ERR_UNSUPPORTED)
__host__ __device__ inline int encoding_bytes_per_pixel(int encoding) {
  switch (encoding) {
    case MPE_ENC_MONO8: return 1;
    case MPE_ENC_MONO16: return 2;
    case MPE_ENC_BGR8: case MPE_ENC_RGB8: return 3;
    case MPE_ENC_BGRA8: case MPE_ENC_RGBA8: return 4;
    default: return 0;
  }
}

}  // namespace mpe
