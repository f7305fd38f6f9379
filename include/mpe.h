/*
 * mpe.h — C ABI of the MI355X (gfx950) compute back-end for the per-frame hot path of
 * uzh-rpg/rpg_monocular_pose_estimator.
 *
 * The reference has no C ABI for this path; its seams are C++.  Every entry
 * point below names the reference interface it replaces (paths relative to the reference root,
 * lib = monocular_pose_estimator_lib).  The library is libmpe_hip.so, built by
 * rpg_monocular_pose_estimator_amd/csrc/Makefile with hipcc --offload-arch=gfx950.
 *
 * Conventions
 *   - plain pointers and sizes only; caller owns every buffer; no exceptions cross the ABI.
 *   - one mpe_handle = one GPU + one HIP stream; a handle is used by one thread at a time
 *     (the reference's PoseEstimator is a single-threaded stateful object too, node.cpp:31).
 *   - return value: 0 = call executed, <0 = usage / HIP error (see mpe_last_error()).
 *     Per-frame outcome is in mpe_result.status: 0 = pose found (estimateBodyPose -> true),
 *     1 = no pose (-> false), <0 = frame exceeded a documented device capacity (never silent).
 *   - matrices are row-major doubles: K[9], T[16] (T_camera_object), cov[36] in twist order
 *     (upsilon, omega) exactly as PoseEstimator::getPoseCovariance() / ROS.cpp:178-187.
 *   - markers: n x 3 doubles (x,y,z) — List4DPoints without the homogeneous 1 (PE.h:351).
 *   - detections: n x 2 doubles, undistorted pixels — List2DPoints (DT.h:50).
 *   - correspondences: rows (marker, detection), 1-based, 0 = none — VectorXuPairs (DT.h:47).
 *   - hist: n_det x n_markers uint32 row-major (row = detection) — hist_corr, PE.cpp:556.
 */
#ifndef MPE_H_
#define MPE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPE_MAX_MARKERS 16    /* object_points_ capacity (reference: unbounded; 32-bit factorial
                                 already overflows at 13, COMB.cpp:34-45 — replicated) */
#define MPE_MAX_DETECTIONS 64 /* detections kept per frame by the ordinary entries; more -> status
                                 MPE_FRAME_TOO_MANY_DETECTIONS.  (The reference has no limit, led_detector.cpp:65-86 /
                                 pose_estimator.cpp:549-557; with 64 detections and 5 markers initialise() already runs
                                 2.5 M P3P solves for one frame.  Frames with more than MPE_FAST_VOTE_DETECTIONS are voted
                                 by the strict loop nest.)  Detection sets of up to MPE_WIDE_DETECTIONS go through the
                                 separate *_wide entries below (mpe_vote_batch_wide, mpe_solve_bruteforce_batch_wide). */
#define MPE_WIDE_DETECTIONS 256 /* detections of one set in the *_wide entries (= MPE_MAX_RAW_BLOBS) */
#define MPE_FAST_VOTE_DETECTIONS 32 /* widest frame the fast voting kernels' 32-bit detection masks hold */
#define MPE_MAX_RAW_BLOBS 256 /* external contours per frame before the shape filter */
#define MPE_MAX_KSIZE 37      /* Gaussian kernel taps: sigma <= 6 (cfg:13) */

/* per-frame status codes (mpe_result.status, mpe_detections.status) */
#define MPE_FRAME_POSE 0
#define MPE_FRAME_NO_POSE 1
#define MPE_FRAME_TOO_MANY_DETECTIONS (-10) /* > MPE_MAX_DETECTIONS blobs passed the filter: the record then holds the
                                               first MPE_MAX_DETECTIONS of the reference's order (OpenCV's contour order)
                                               — unless more than 512 passed, when WHICH blobs it holds is unspecified
                                               (the general blob tier keeps 512, appended concurrently) */
#define MPE_FRAME_TOO_MANY_BLOBS (-11)      /* > MPE_MAX_RAW_BLOBS external contours */
#define MPE_FRAME_TOO_MANY_ROWS (-12)       /* bright rows exceed the LDS band capacity */
#define MPE_FRAME_VOTE_LIST_FULL (-13)      /* internal since round 5: hypotheses left to the strict arithmetic did not fit
                                               their list; such a frame is voted again by the strict loop nest before the
                                               tail and comes out with an ordinary status (never returned to a caller) */

/* call-level error codes */
#define MPE_OK 0
#define MPE_ERR_ARG (-1)
#define MPE_ERR_HIP (-2)
#define MPE_ERR_UNSUPPORTED (-3)
#define MPE_ERR_NO_DEVICE (-4)

typedef struct mpe_handle mpe_handle;

/* Mirrors the tuning members of PoseEstimator (PE.h:68-72, 85-91) and the dynamic-reconfigure
 * contract (monocular_pose_estimator/cfg/MonocularPoseEstimator.cfg:12-22). */
typedef struct mpe_params {
  int threshold_value;                      /* detection_threshold_value_ */
  double gaussian_sigma;                    /* gaussian_sigma_ */
  double min_blob_area;                     /* min_blob_area_ */
  double max_blob_area;                     /* max_blob_area_ */
  double max_width_height_distortion;       /* max_width_height_distortion_ */
  double max_circular_distortion;           /* max_circular_distortion_ */
  double back_projection_pixel_tolerance;   /* setBackProjectionPixelTolerance, PE.h:483 */
  double nearest_neighbour_pixel_tolerance; /* setNearestNeighbourPixelTolerance, PE.h:503 */
  double certainty_threshold;               /* setCertaintyThreshold, PE.h:523 */
  double valid_correspondence_threshold;    /* setValidCorrespondenceThreshold, PE.h:543 */
  unsigned roi_border_thickness;            /* roi_border_thickness_ (tracking path only) */
  unsigned histogram_threshold;             /* 0 -> numCombinations(n_markers,3) as PE.cpp:54 */
} mpe_params;

typedef struct mpe_result {
  double T[16];      /* getPredictedPose(), PE.h:406 */
  double cov[36];    /* getPoseCovariance(), PE.h:416 */
  int status;        /* MPE_FRAME_* */
  int n_det;         /* detections that passed the blob filter */
  int n_corr;        /* rows of correspondences_ after correspondencesFromHistogram */
  int gn_iterations; /* Gauss-Newton iterations used by optimisePose */
} mpe_result;

typedef struct mpe_detections {
  int n;      /* min(number of detections, MPE_MAX_DETECTIONS) */
  int status; /* 0 or MPE_FRAME_TOO_MANY_* */
  double undist_xy[2 * MPE_MAX_DETECTIONS]; /* pixel_positions of findLeds (LED.h:84-88); entries 2 n .. are unspecified */
  float dist_xy[2 * MPE_MAX_DETECTIONS];    /* distorted_detection_centers; entries 2 n .. are unspecified */
} mpe_detections;

/* mpe_detections with room for MPE_WIDE_DETECTIONS points: the record of the *_wide entries */
typedef struct mpe_detections_wide {
  int n;      /* min(number of detections, MPE_WIDE_DETECTIONS) */
  int status; /* 0 or MPE_FRAME_TOO_MANY_* */
  double undist_xy[2 * MPE_WIDE_DETECTIONS]; /* entries 2 n .. are unspecified */
  float dist_xy[2 * MPE_WIDE_DETECTIONS];    /* entries 2 n .. are unspecified */
} mpe_detections_wide;

/* fills *p with the parameter set of launch/demo.launch:12-22 */
void mpe_default_params(mpe_params* p);

/* device < 0: use the current HIP device.  Fails (MPE_ERR_NO_DEVICE) when no gfx950 GPU is
 * visible — there is no CPU fallback. */
int mpe_create(mpe_handle** out, int device);
void mpe_destroy(mpe_handle* h);
const char* mpe_last_error(const mpe_handle* h);
/* Use an existing hipStream_t (e.g. a torch.cuda.Stream); NULL restores the handle's own non-blocking
 * stream (it does NOT select the legacy default stream). */
int mpe_set_stream(mpe_handle* h, void* hip_stream);
void* mpe_get_stream(mpe_handle* h);
int mpe_synchronize(mpe_handle* h);

/* ≙ LEDDetector::findLeds (lib/include/.../led_detector.h:84-88, lib/src/led_detector.cpp:35-112)
 * on ONE host frame: threshold -> Gaussian blur -> external contours -> polygon area/moments ->
 * shape filter -> undistortPoints.  undist_xy / dist_xy hold 2*cap values. */
int mpe_find_leds(mpe_handle* h, const uint8_t* img, int rows, int cols, size_t stride_bytes,
                  int roi_x, int roi_y, int roi_w, int roi_h, const mpe_params* p,
                  const double K[9], const double* D, int nD, double* undist_xy, float* dist_xy,
                  int cap, int* n_out);

/* ≙ PoseEstimator::setImagePoints + initialise + optimiseAndUpdatePose on a fresh estimator
 * (lib/include/.../pose_estimator.h:425,749,773; lib/src/pose_estimator.cpp:80-91,544-721,
 * 733-812).  hist (n_det*n_markers) and corr (2*n_markers) are optional outputs. */
int mpe_solve_bruteforce(mpe_handle* h, const double* det_xy, int n_det, const double* markers_xyz,
                         int n_markers, const double K[9], const mpe_params* p, mpe_result* out,
                         uint32_t* hist, uint32_t* corr);
/* PoseEstimator::initialise() alone (pose_estimator.h:749, pose_estimator.cpp:544-721): voting,
 * correspondencesFromHistogram and checkCorrespondences WITHOUT the Gauss-Newton refinement — out->T is
 * the pose of computeTransformation, out->cov zero.  Same arguments as mpe_solve_bruteforce. */
int mpe_initialise(mpe_handle* h, const double* det_xy, int n_det, const double* markers_xyz, int n_markers,
                   const double K[9], const mpe_params* p, mpe_result* out, uint32_t* hist, uint32_t* corr);

/* ≙ PoseEstimator::estimateBodyPose (pose_estimator.h:366, pose_estimator.cpp:62-96) on a FRESH
 * estimator per frame (it_since_initialized_ == 0: whole-image detection + brute-force
 * initialisation) for a batch of independent frames — the measured entry point.
 * frames: n_frames images, frame f at frames + f*frame_stride_bytes, rows of stride_bytes.
 * frames_on_device != 0: `frames` is a device pointer (results is still a HOST pointer). */
int mpe_estimate_batch(mpe_handle* h, const uint8_t* frames, int n_frames, int rows, int cols,
                       size_t stride_bytes, size_t frame_stride_bytes, int frames_on_device,
                       const double* markers_xyz, int n_markers, const double K[9],
                       const double* D, int nD, const mpe_params* p, mpe_result* results);

/* ---- frame decode (SURVEY 8f "input side") -------------------------------------------------------------
 * ≙ cv_bridge::toCvCopy(image_msg, sensor_msgs::image_encodings::MONO8) (monocular_pose_estimator.cpp:147) for the
 * encodings a camera driver publishes: the payload of n_frames sensor_msgs/Image messages (rows x cols pixels, rows of
 * src_stride_bytes = Image.step, frame f at src + f * src_frame_stride_bytes) -> packed mono8 frames (rows x cols bytes
 * each, stride = cols), which is what every other entry point takes.  src / dst may each be a host or a device pointer.
 *   MPE_ENC_BGR8 / RGB8 / BGRA8 / RGBA8: cv::cvtColor(..., COLOR_{BGR,RGB,BGRA,RGBA}2GRAY) on CV_8U:
 *       Y = (B * 1868 + G * 9617 + R * 4899 + 2^13) >> 14   (integer, bit-exact)
 *       — the 14-bit weights of OpenCV 2.4 and 3.0 .. 3.4.1, the versions the reference's ROS Indigo / Kinetic ship.
 *       OpenCV >= 3.4.2 / 4.x use 15-bit weights (9798, 19235, 3735, >> 15) and can differ by one gray level: a caller
 *       linked against one of those keeps cv_bridge for colour frames (compat/ros/mpe_ros_glue.cpp does, unless built
 *       with -DMPE_OPENCV_GRAY_14BIT)
 *   MPE_ENC_MONO16: cv::Mat::convertTo(CV_8U, 255. / 65535.) = saturate_cast<uchar>((float)v * (float)(255. / 65535.)),
 *       after cv_bridge's byte swap when Image.is_bigendian differs from the host (src_big_endian)
 *   MPE_ENC_MONO8: a (strided) copy.
 *   MPE_ENC_YUV422 (U Y V Y) / MPE_ENC_YUV422_YUY2 (Y U Y V), two source bytes per pixel: cvtColor(...,
 *       COLOR_YUV2GRAY_UYVY / _YUY2) — the gray value is the pixel's Y byte (byte 1 of its pair / byte 0), an exact copy
 *       in every OpenCV.  Odd cols are legal.
 *   MPE_ENC_BAYER_RGGB8 / BGGR8 / GBRG8 / GRBG8, one source byte per pixel; the name gives the colours of the image
 *       pixels (0,0), (0,1), (1,0), (1,1): cvtColor(..., COLOR_Bayer{BG,RG,GR,GB}2GRAY), OpenCV's SCALAR Bayer2Gray with
 *       the 14-bit weights R 4899, G 9617, B 1868, every neighbour weighted by the weight of its own colour:
 *         red or blue site, centre c of colour X, the four diagonal neighbours of the other colour Z:
 *           Y = (wZ * (four diagonal neighbours) + 9617 * (four edge neighbours) + 4 * wX * c + 2^15) >> 16
 *         green site, wV / wH the weights of the colours above-below / left-right:
 *           Y = (wV * (up + down) + wH * (left + right) + 2 * 9617 * c + 2^14) >> 15
 *       Only interior pixels are computed: output pixel (r, c) is the value at (clamp(r, 1, rows - 2),
 *       clamp(c, 1, cols - 2)), so the border rows and columns repeat their inner neighbours, as OpenCV's do; an image
 *       with rows < 3 or cols < 3 decodes to all zeros.  This is a restatement nothing reference-held pins (the
 *       reference calls cv_bridge::toCvCopy(..., MONO8) and was never run on Bayer frames here), and OpenCV's SIMD
 *       path for this conversion rounds per term and can differ from its scalar path by one gray level: a caller who
 *       needs the linked OpenCV's bytes keeps cv_bridge for Bayer frames (compat/ros/mpe_ros_glue.cpp does, unless
 *       built with -DMPE_OPENCV_BAYER_SCALAR).
 * 16-bit Bayer and every code outside {0 .. 5, 16 .. 21}: MPE_ERR_UNSUPPORTED.  The entries that take HOST frames beside
 * an encoding (mpe_track_step_batch_wide, the *_formats entries) decode device frames alone: host frames in a Bayer or
 * YUV encoding are MPE_ERR_UNSUPPORTED there (what these codes answered before they existed), in one of the other five
 * non-mono8 encodings MPE_ERR_ARG as ever. */
#define MPE_ENC_MONO8 0
#define MPE_ENC_BGR8 1
#define MPE_ENC_RGB8 2
#define MPE_ENC_BGRA8 3
#define MPE_ENC_RGBA8 4
#define MPE_ENC_MONO16 5
#define MPE_ENC_BAYER_RGGB8 16 /* sensor_msgs "bayer_rggb8" -> cv::COLOR_BayerBG2GRAY */
#define MPE_ENC_BAYER_BGGR8 17 /* "bayer_bggr8" -> COLOR_BayerRG2GRAY */
#define MPE_ENC_BAYER_GBRG8 18 /* "bayer_gbrg8" -> COLOR_BayerGR2GRAY */
#define MPE_ENC_BAYER_GRBG8 19 /* "bayer_grbg8" -> COLOR_BayerGB2GRAY */
#define MPE_ENC_YUV422 20      /* "yuv422" = U Y V Y  -> COLOR_YUV2GRAY_UYVY */
#define MPE_ENC_YUV422_YUY2 21 /* "yuv422_yuy2" = Y U Y V -> COLOR_YUV2GRAY_YUY2 */
int mpe_convert_to_mono8(mpe_handle* h, const void* src, int src_on_device, int encoding, int src_big_endian, int n_frames,
                         int rows, int cols, size_t src_stride_bytes, size_t src_frame_stride_bytes, uint8_t* dst,
                         int dst_on_device);

/* Page-locked host memory for frame buffers (what a camera driver / cv_bridge::toCvCopy target should write into,
 * monocular_pose_estimator.cpp:147): with HOST frames in pinned memory mpe_estimate_batch ingests a large batch
 * in chunks (option "ingest_chunk", default 2048 frames, 0 = one copy), the H2D copy of chunk c + 1 running
 * beside the kernels of chunk c — the call is then bound by the PCIe link alone.  NULL on failure. */
void* mpe_alloc_pinned(size_t bytes);
void mpe_free_pinned(void* p);

/* ---- the same entry point over SEVERAL GPUs of one node, from ONE host process ----
 * Frames are independent on this branch (pose_estimator.cpp:68-91 reads no estimator state when
 * it_since_initialized_ < 1), so the batch shards into contiguous chunks — shard d of n_dev gets frames
 * [lo, hi) as mpe_shard_bounds says (sizes differ by at most one frame) — with NO exchange step between the
 * devices; the only "gather" is that every shard's pose records land in the caller's ONE host array, in
 * frame order.  handles[d]: n_dev DISTINCT handles (normally created on n_dev different devices; several
 * handles on one device work too).  One host thread per shard drives that handle's mpe_estimate_batch.
 * Returns 0, or the first failing shard's error code (text: mpe_last_error of that shard's handle).
 * (One process per GPU + a pose gather over RCCL, as bench.py and rpg_monocular_pose_estimator_amd/parallel.py
 * do it, is the other way to use N GPUs; results are identical.) */
void mpe_shard_bounds(int n_frames, int shard, int n_shards, int* lo, int* hi);
/* host frames: frame f at frames + f*frame_stride_bytes, copied to the shard's device by its own thread */
int mpe_estimate_batch_multi(mpe_handle* const* handles, int n_dev, const uint8_t* frames, int n_frames,
                             int rows, int cols, size_t stride_bytes, size_t frame_stride_bytes,
                             const double* markers_xyz, int n_markers, const double K[9], const double* D,
                             int nD, const mpe_params* p, mpe_result* results);
/* device-resident shards: d_frames[d] = n_frames[d] packed frames (cols % 16 == 0, 16-byte aligned) in the
 * memory of handles[d]'s device; results = one HOST array of sum(n_frames) records, shard after shard */
int mpe_estimate_batch_multi_device(mpe_handle* const* handles, int n_dev, const uint8_t* const* d_frames,
                                    const int* n_frames, int rows, int cols, const double* markers_xyz,
                                    int n_markers, const double K[9], const double* D, int nD,
                                    const mpe_params* p, mpe_result* results);

/* The same with the gather ON THE DEVICES: every shard's pose records travel from its GPU into ONE device-resident
 * array on handles[0]'s device (sum(n_frames) records, shard after shard) — over RCCL (ncclCommInitAll once per device
 * list, one grouped ncclSend / ncclRecv exchange per call: point-to-point over xGMI, 432 bytes per frame, no host
 * copy) when the handles sit on distinct devices, by plain device-to-device copies when several handles share a
 * device.  *used_rccl (optional) tells which.  RCCL is loaded at first use (dlopen of librccl.so); MPE_ERR_UNSUPPORTED
 * if it cannot be found.  Blocking: the records are complete when the call returns. */
int mpe_estimate_batch_multi_device_gather(mpe_handle* const* handles, int n_dev, const uint8_t* const* d_frames,
                                           const int* n_frames, int rows, int cols, const double* markers_xyz,
                                           int n_markers, const double K[9], const double* D, int nD,
                                           const mpe_params* p, mpe_result* d_results_dev0, int* used_rccl);

/* Streaming entry, see mpe_estimate_batch_device_submit below: `hip_event` (a hipEvent_t, or NULL) marks the point at
 * which the frames the NEXT _submit call announces (d_next_frames) are final; one-shot, consumed by that _submit. */
int mpe_stream_next_ready(mpe_handle* h, void* hip_event);
/* ... and: forget what the last submission scanned ahead (the announced buffer has been rewritten since). */
int mpe_stream_drop_prefetch(mpe_handle* h);

/* Fully asynchronous variant for device-resident pipelines: frames AND results are device
 * pointers, nothing is copied, the call only enqueues kernels on the handle's stream.
 * frames must be 16-byte aligned with cols % 16 == 0, stride_bytes == cols and
 * frame_stride_bytes == rows*cols (the packed layout).
 * Ordering: the call behaves like ONE operation on the handle's stream — its kernels start after
 * everything enqueued on that stream before the call (large batches fork onto internal side
 * streams and join back) and d_results is complete for anything enqueued on it afterwards.  Work
 * on OTHER streams, including the legacy default stream 0, is not ordered with it: share a real
 * stream through mpe_set_stream (a NULL argument means the handle's own stream, NOT stream 0). */
int mpe_estimate_batch_device(mpe_handle* h, const uint8_t* d_frames, int n_frames, int rows,
                              int cols, const double* markers_xyz, int n_markers,
                              const double K[9], const double* D, int nD, const mpe_params* p,
                              mpe_result* d_results);

/* The same for a STREAM of device-resident batches (a camera pipeline that keeps frames coming): _submit only enqueues,
 * and it does not join the library's internal side streams back into the handle's stream — the records of the
 * submission are complete when the event behind _collect says so, not at a point of the handle's stream.  _collect
 * makes `hip_stream` (NULL = the handle's stream) wait for the records of the OLDEST un-collected submission; use the
 * stream that consumes them (a D2H copy, a pose gather) so that the next batch's kernels need not wait for it.
 * Up to two submissions may be in flight (submit k, submit k+1, collect k, ...); d_results must stay valid and
 * untouched until its submission has been collected and the consumer stream has passed that point.
 * d_next_frames / n_next_frames (optional): the frames of the NEXT submission (same geometry, camera, parameters).
 * The last voting launch of this submission then also scans the next one's first sub-batch, and the next _submit with
 * exactly those frames skips that scan — in steady state no kernel of a batch runs without an image scan beside it
 * (pose_estimator.cpp:62-96 has no counterpart: the reference handles one frame at a time).  A hint that does not come
 * true only costs the wasted scan.  mpe_estimate_batch_device = _submit without a hint + _collect on the handle's
 * stream; it refuses to run while a submission is un-collected.
 * CONTRACT for an announced buffer: its pixels are READ by this submission's last launches (on the handle's stream and
 * on an internal side stream), i.e. possibly long before the next _submit.  They must therefore (a) be final, in the
 * order of the handle's stream, when this _submit is called — or, if they are still being written on another stream
 * (the upload of batch k+1 while batch k runs), the caller passes the event that marks their completion through
 * mpe_stream_next_ready(h, event) right BEFORE this _submit: the reading launches then wait for it — and (b) stay
 * unmodified until the next _submit has been called.  A buffer that was rewritten in between (a double-buffered camera
 * pipeline that re-uses it) must be withdrawn with mpe_stream_drop_prefetch(h) before the next _submit, which then
 * scans it again; the library recognises a prefetched batch by POINTER and shape only and cannot see the rewrite. */
int mpe_estimate_batch_device_submit(mpe_handle* h, const uint8_t* d_frames, int n_frames, int rows, int cols,
                                     const double* markers_xyz, int n_markers, const double K[9], const double* D,
                                     int nD, const mpe_params* p, mpe_result* d_results,
                                     const uint8_t* d_next_frames, int n_next_frames);
int mpe_estimate_batch_device_collect(mpe_handle* h, void* hip_stream);

/* ≙ PoseEstimator::setCorrespondences + checkCorrespondences + optimiseAndUpdatePose
 * (pose_estimator.h:463,724,773; pose_estimator.cpp:394-542,733-812) — the tracking path's
 * validate-and-refine step for correspondences found by nearest neighbour.  corr: n_corr rows
 * (marker, detection), 1-based.  out->status: 0 pose, 1 correspondences rejected. */
int mpe_check_and_refine(mpe_handle* h, const double* det_xy, int n_det, const double* markers_xyz,
                         int n_markers, const double K[9], const mpe_params* p, const uint32_t* corr,
                         int n_corr, mpe_result* out);

/* The two halves of the call above as separate stage entry points (same kernel, other instantiations):
 * PoseEstimator::checkCorrespondences (pose_estimator.h:724, pose_estimator.cpp:394-542) — out->status 0
 * and out->T = the UNREFINED pose of computeTransformation when the correspondences validate, else 1;
 * PoseEstimator::optimisePose (pose_estimator.h:773, pose_estimator.cpp:733-792) — Gauss-Newton from
 * T_init on the given correspondences (no validation): out->T, out->cov, out->gn_iterations; status 1
 * when fewer than 3 correspondences were given (singular normal equations). */
int mpe_check_correspondences(mpe_handle* h, const double* det_xy, int n_det, const double* markers_xyz,
                              int n_markers, const double K[9], const mpe_params* p, const uint32_t* corr,
                              int n_corr, mpe_result* out);
int mpe_optimise_pose(mpe_handle* h, const double* det_xy, int n_det, const double* markers_xyz, int n_markers,
                      const double K[9], const mpe_params* p, const uint32_t* corr, int n_corr,
                      const double T_init[16], mpe_result* out);

/* ---- static primitives of the reference, batched (n independent problems, one GPU lane each) ----
 * P3P::computePoses (p3p.h:110, p3p.cpp:65-236): feature_vectors / world_points n x 9, point i of a
 * problem at [3i..3i+2] (= column i of the reference's 3x3 matrices); solutions n x 48 = 4 solutions
 * x 3x4 row-major [R|C]; status[i] 0, or -1 for collinear world points (solutions[i] untouched). */
int mpe_p3p_batch(mpe_handle* h, const double* feature_vectors, const double* world_points, int n,
                  double* solutions, int* status);
/* P3P::solveQuartic (p3p.h:127, p3p.cpp:238-286): factors n x 5 (highest power first), real_roots n x 4
 * (real parts of the four complex Ferrari roots, like the reference).  variant 0 = IEEE operators
 * (as the validation kernel uses it), 1 = the voting kernel's literal-order variant,
 * 2 = the three complex powers as libstdc++ / glibc evaluate them (solve_quartic_glibc, the function
 * the strict voting item of "vote_arith" 3 / 4 calls).  Any other variant: MPE_ERR_ARG. */
int mpe_solve_quartic_batch(mpe_handle* h, const double* factors, int n, int variant, double* real_roots);
/* The stage-level parity entry of csrc/mpe_ddmath.h (the libstdc++ / glibc restatement behind "vote_arith"
 * 3 / 4): primitive `which` at the n argument pairs (a[i], b[i]), out n x 2 = (out0, out1) per pair.
 * Selectors (csrc/mpe_ddmath_eval.h; one argument: b is read and ignored, one result: out1 = 0):
 * 0 log, 1 log1p (correctly rounded), 2 exp, 3 sin, 4 cos, 5 hypot_g(a, b), 6 atan2(y = a, x = b),
 * 7 pow(a, b), 8 log1p_g; 9 clog_g(re = a, im = b); 10 / 11 / 12 cpow_g(re = a, im = b, y) at y = 1/3,
 * 2, 3; 13 the quartic's complex square root; 14 x2y2m1_g(a, b); the unrounded double-double pairs
 * (hi, lo) with x = the exact product a b and y = the exact sum a + b: 15 x, 16 x + y, 17 x y, 18 x / y,
 * 19 sqrt x, 20 log x, 21 exp x, 22 atan x, 23 / 24 the sine / cosine of a before their one rounding.
 * It exists for tests that hold the device build of that header to the bits of its host build; nothing
 * on the estimation path calls it.  n == 0: MPE_OK; a selector outside 0 .. MPE_DDMATH_SELECTORS - 1,
 * n < 0 or a null pointer with n > 0: MPE_ERR_ARG (the handle stays usable). */
#define MPE_DDMATH_SELECTORS 25
int mpe_ddmath_batch(mpe_handle* h, int which, const double* a, const double* b, int n, double* out);

/* LEDDetector::determineROI (led_detector.h:105, led_detector.cpp:114-179): bounding box of the predicted
 * (undistorted) pixel positions, its two corners distorted, grown by border_size, clipped to the
 * image; the whole image when the box degenerates.  Host arithmetic (a dozen flops), no device. */
int mpe_determine_roi(const double* pixel_positions, int n_points, int rows, int cols, int border_size,
                      const double K[9], const double* D, int nD, int roi_xywh[4]);
/* LEDDetector::distortPoints (led_detector.h:135, led_detector.cpp:181-224), float in / float out. */
int mpe_distort_points(const float* src_xy, float* dst_xy, int n, const double K[9], const double* D, int nD);

/* One frame of the tracking branch as ONE device submission (pose_estimator.cpp:98-110 + 831-839):
 * LEDDetector::findLeds inside the ROI, then — when at least 4 LEDs were found — findCorrespondences
 * (nearest detection of every predicted marker pixel within nearest_neighbour_pixel_tolerance,
 * pose_estimator.cpp:372-392), checkCorrespondences and optimisePose.  img is a HOST image; the ROI is
 * packed into pinned memory and sent with the predicted pixels in one copy, the detections,
 * correspondences and pose come back in one copy.  predicted_px: n_markers x 2 (undistorted pixels).
 * dets_out: what findLeds found (always written); corr_out: 2*MPE_MAX_MARKERS uint32, rows
 * (marker, detection) 1-based, out->n_corr rows valid; out->status 0 = pose refined, 1 = fewer than
 * 4 LEDs or correspondences rejected (the caller then retries / re-initialises as the reference does),
 * <0 = a device capacity was exceeded.  The submission is that of mpe_track_step_batch with one item (refused, like
 * _submit, while a lock-step submission of the handle is pending); mpe_tracker_estimate makes the same submissions
 * through mpe_track_step_batch_setups_submit / _collect. */
int mpe_track_step(mpe_handle* h, const uint8_t* img, int rows, int cols, size_t stride_bytes, int roi_x,
                   int roi_y, int roi_w, int roi_h, const mpe_params* p, const double K[9], const double* D,
                   int nD, const double* markers_xyz, int n_markers, const double* predicted_px,
                   mpe_detections* dets_out, uint32_t* corr_out, mpe_result* out);

/* ---- lock-step batches over N independent camera streams (BASELINE configs[4]) ----------------------
 * mpe_track_step for frame k of N streams in ONE device submission: every stream's ROI goes into one slot of
 * a uniform slot array (zero beyond the ROI; the blob kernels read the window size / origin per slot, so image
 * borders and centroid offsets are those of the stand-alone clone of led_detector.cpp:44), one image scan, one
 * blob extraction and one validate / refine kernel pair run over the N slots, one copy returns N records.
 * All streams share rows / cols / stride, camera, marker set and parameters (streams of different set-ups:
 * mpe_track_step_batch_setups below).  predicted_px == NULL for an
 * item = detection only (out[i].status = 1).  Group items of very different ROI size into separate calls:
 * the slot is as large as the largest ROI of the call.  dets_out n, corr_out n x 2*MPE_MAX_MARKERS, out n. */
typedef struct mpe_track_item {
  const uint8_t* img;          /* HOST image of this stream (a DEVICE pointer in the *_device entries below) */
  int roi_x, roi_y, roi_w, roi_h;
  const double* predicted_px;  /* n_markers x 2 undistorted pixels, or NULL */
} mpe_track_item;
int mpe_track_step_batch(mpe_handle* h, const mpe_track_item* items, int n, int rows, int cols, size_t stride_bytes,
                         const mpe_params* p, const double K[9], const double* D, int nD,
                         const double* markers_xyz, int n_markers, mpe_detections* dets_out, uint32_t* corr_out,
                         mpe_result* out);
/* The same in two halves, for callers that overlap the host work of one group of streams with the device work of
 * another: _submit packs the ROIs and enqueues copy-in, kernels and copy-out on the handle's stream WITHOUT waiting;
 * _collect waits and hands out the records of that submission (one outstanding submission per handle). */
int mpe_track_step_batch_submit(mpe_handle* h, const mpe_track_item* items, int n, int rows, int cols,
                                size_t stride_bytes, const mpe_params* p, const double K[9], const double* D, int nD,
                                const double* markers_xyz, int n_markers);
int mpe_track_step_batch_collect(mpe_handle* h, mpe_detections* dets_out, uint32_t* corr_out, mpe_result* out);
/* _collect without a submission in flight is an error (MPE_ERR_ARG: a caller that missed a failed _submit must not read
 * records that were never written).  _cancel abandons the submission in flight, if any: it waits for the device and
 * frees the handle for the next _submit / mpe_track_step (used on error paths that drive several handles). */
int mpe_track_step_batch_cancel(mpe_handle* h);
/* Lock-step batches whose streams differ in camera, marker set and parameters: every physical camera of a rig has its own
 * K / D (the reference: one PoseEstimator per camera, each with its own calibration and object,
 * pose_estimator.h:63,82-83, filled per node from that camera's camera_info, monocular_pose_estimator.cpp:103-120).
 * A set-up is one such camera + marker set + parameter set (n_markers 1 .. MPE_MAX_MARKERS); item i runs with
 * setups[item_setup[i]].  All items share rows / cols / stride (items that differ in
 * them: mpe_track_step_batch_formats below).  Each item's records are byte-identical to those of
 * mpe_track_step_batch over the items of its set-up alone.  Records come back in the caller's item order; the fused time
 * step stays ONE launch for the whole submission (set-ups of more than 8 markers, track_fused 0 and slots that overflow
 * the small blob tier run per set-up through the chain of kernels).  mpe_track_step_batch_collect / _cancel serve this
 * submit too.  MPE_ERR_ARG before any device work on a null pointer, a set-up index out of range, n_markers above
 * MPE_MAX_MARKERS or a ROI outside the image. */
typedef struct mpe_track_setup {
  const mpe_params* p;
  const double* K;            /* 3x3 row-major */
  const double* D;            /* nD distortion coefficients (may be NULL when nD == 0) */
  int nD;
  const double* markers_xyz;  /* n_markers x 3 */
  int n_markers;
} mpe_track_setup;
int mpe_track_step_batch_setups(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n, int rows,
                                int cols, size_t stride_bytes, const mpe_track_setup* setups, int n_setups,
                                mpe_detections* dets_out, uint32_t* corr_out, mpe_result* out);
int mpe_track_step_batch_setups_submit(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n,
                                       int rows, int cols, size_t stride_bytes, const mpe_track_setup* setups,
                                       int n_setups);
/* mpe_track_step_batch_setups[_submit] for streams whose frames are already in DEVICE memory (a decoder, a simulator,
 * a replay buffer, mpe_convert_to_mono8 with a device destination): items[i].img is a device pointer here, the struct
 * is unchanged.  Instead of cloning every ROI on the host and copying the pixels (what the entries above do), the
 * submission copies only its small header and a kernel gathers the ROIs from the caller's images into the same slots,
 * byte for byte; everything behind that is the same submission, so the records are byte-identical to those of
 * mpe_track_step_batch_setups over the same frames in host memory, and mpe_track_step_batch_collect / _cancel serve
 * this submit too.  item_setup == NULL with n_setups == 1 is a uniform batch (there is no separate uniform entry).
 * Every img must lie, with its whole image (to the last pixel of row rows - 1), inside one device allocation on the
 * handle's device: host memory — pinned memory included — is refused with MPE_ERR_ARG before anything is submitted
 * (the host entries are for that); the other usage errors are those of mpe_track_step_batch_setups_submit.
 * Ordering: the gather runs on the handle's stream.  The frames must be final in that stream's order when _submit is
 * called (as with mpe_estimate_batch_device) and must stay unmodified until _collect / _cancel has returned: a slot
 * that overflows the small blob tier is re-run from the gathered slots, but a retry by the caller reads them again. */
int mpe_track_step_batch_setups_device(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n,
                                       int rows, int cols, size_t stride_bytes, const mpe_track_setup* setups,
                                       int n_setups, mpe_detections* dets_out, uint32_t* corr_out, mpe_result* out);
int mpe_track_step_batch_setups_device_submit(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n,
                                              int rows, int cols, size_t stride_bytes, const mpe_track_setup* setups,
                                              int n_setups);
/* mpe_track_step_batch_setups_device[_submit] for device frames in the camera's own ENCODING (a decoder or a DMA engine
 * that delivers bgr8, mono16, ... into device memory): `encoding` is one MPE_ENC_* value for the whole call, as rows,
 * cols and the stride are (items that differ in them: mpe_track_step_batch_formats below); src_big_endian has the
 * meaning it has in mpe_convert_to_mono8 (read for MPE_ENC_MONO16 alone).  stride_bytes is in SOURCE bytes (Image.step); rows, cols and every ROI stay in pixels; items[i].img needs no
 * alignment.  The gather kernel decodes the pixels it gathers, by the rules stated at mpe_convert_to_mono8, so no mono8
 * copy of the frames is made and no separate conversion is launched: every detection record, correspondence row and
 * result is byte-identical to what mpe_track_step_batch_setups_device returns over the same frames after
 * mpe_convert_to_mono8 with a device destination (and so to the host entries' records over the converted frames).
 * MPE_ENC_MONO8 is handed to mpe_track_step_batch_setups_device_submit as it is.  mpe_track_step_batch_collect / _cancel
 * serve this submit too; ordering as above.  Usage errors, all before any device work: whatever
 * mpe_track_step_batch_setups_device_submit refuses (every img must lie, with its whole ENCODED image —
 * (rows - 1) * stride_bytes + cols * bytes per pixel —, inside one device allocation on the handle's device);
 * stride_bytes < cols * bytes per pixel: MPE_ERR_ARG; an encoding outside MPE_ENC_* (16-bit Bayer, ...): MPE_ERR_UNSUPPORTED, as
 * mpe_convert_to_mono8 answers it. */
int mpe_track_step_batch_setups_device_encoded(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n,
                                               int rows, int cols, size_t stride_bytes, int encoding, int src_big_endian,
                                               const mpe_track_setup* setups, int n_setups, mpe_detections* dets_out,
                                               uint32_t* corr_out, mpe_result* out);
int mpe_track_step_batch_setups_device_encoded_submit(mpe_handle* h, const mpe_track_item* items, const int* item_setup,
                                                      int n, int rows, int cols, size_t stride_bytes, int encoding,
                                                      int src_big_endian, const mpe_track_setup* setups, int n_setups);
/* The lock-step time step of streams that differ in IMAGE FORMAT — one PoseEstimator per camera (pose_estimator.h:63,
 * 82-83), each fed its own camera_info and its own image encoding (monocular_pose_estimator.cpp:103-126,147): a 752 x 480
 * mono camera beside a 1920 x 1200 one, a bgr8 camera beside a mono16 one, one sensor behind drivers with different row
 * padding.  Item i is an image of formats[item_format[i]] — rows, cols, the stride in SOURCE bytes (Image.step), one
 * MPE_ENC_* value and, for MPE_ENC_MONO16 alone, the byte order — and runs with setups[item_setup[i]]; its ROI is in
 * pixels of its own image.  item_format == NULL only with n_formats == 1, item_setup == NULL only with n_setups == 1.
 * frames_on_device 0: items[i].img are host frames, packed with the item's own stride; every format that has items
 * must be MPE_ENC_MONO8 (else MPE_ERR_ARG, the rule of mpe_track_step_batch_wide).  1: device frames; ONE gather kernel
 * reads every item by its own format (stride, image end, decode) from a small format table that travels in the same
 * host-to-device copy as the header and the gather table, so the submission is still one copy and one launch in front
 * of the tracking launch.  A call whose items all have one format (equal formats count once) is handed to
 * mpe_track_step_batch_setups_submit / mpe_track_step_batch_setups_device_encoded_submit as it is.  Every item's
 * detections, correspondence rows and result equal, byte for byte, those of the entry of its kind over the items of its
 * format alone (the slot size, the largest ROI of the call, does not enter the records).  mpe_track_step_batch_collect
 * and _cancel serve this submit like every other one.
 * Usage errors, all before any device work, the handle usable afterwards.  MPE_ERR_ARG: a null pointer; a format or
 * set-up index out of range; rows < 1, cols < 1 or stride_bytes < cols * bytes per pixel; a ROI outside ITS OWN image
 * (one that fits the largest image of the call but not the item's never reaches the gather); frames_on_device 1 and an
 * img that does not lie, with its OWN encoded image — (rows - 1) * stride_bytes + cols * bytes per pixel —, inside one
 * device allocation on the handle's device (host memory, pinned included); a submission that is not yet collected.
 * MPE_ERR_UNSUPPORTED: an encoding outside MPE_ENC_*.  n == 0: MPE_OK, nothing submitted. */
typedef struct mpe_image_format {
  int rows, cols;      /* pixels */
  size_t stride_bytes; /* SOURCE bytes per row (Image.step) */
  int encoding;        /* MPE_ENC_* */
  int src_big_endian;  /* read for MPE_ENC_MONO16 alone */
} mpe_image_format;
int mpe_track_step_batch_formats_submit(mpe_handle* h, const mpe_track_item* items, const int* item_setup,
                                        const int* item_format, int n, const mpe_image_format* formats, int n_formats,
                                        int frames_on_device, const mpe_track_setup* setups, int n_setups);
int mpe_track_step_batch_formats(mpe_handle* h, const mpe_track_item* items, const int* item_setup, const int* item_format,
                                 int n, const mpe_image_format* formats, int n_formats, int frames_on_device,
                                 const mpe_track_setup* setups, int n_setups, mpe_detections* dets_out, uint32_t* corr_out,
                                 mpe_result* out);
/* mpe_solve_bruteforce for N detection sets in one submission (the re-initialisations of a lock-step batch):
 * det_xy n x MPE_MAX_DETECTIONS x 2 (n_det[i] valid rows); hist (optional) n x MPE_MAX_DETECTIONS x
 * MPE_MAX_MARKERS, corr (optional) n x 2*MPE_MAX_MARKERS. */
int mpe_solve_bruteforce_batch(mpe_handle* h, const double* det_xy, const int* n_det, int n,
                               const double* markers_xyz, int n_markers, const double K[9], const mpe_params* p,
                               mpe_result* out, uint32_t* hist, uint32_t* corr);
/* mpe_solve_bruteforce_batch for detection sets that differ in camera, marker set and parameters:
 * item i runs with setups[item_setup[i]] (mpe_track_setup; its D / nD are not read here).
 * det_xy n x MPE_MAX_DETECTIONS x 2, n_det[i] valid rows; hist (optional) n x MPE_MAX_DETECTIONS x
 * MPE_MAX_MARKERS, corr (optional) n x 2*MPE_MAX_MARKERS; records in the caller's item order.
 * Every item's record, correspondence rows and histogram are byte-identical to what mpe_solve_bruteforce_batch returns
 * for the items of its set-up alone, under the handle's current options.  Items of two or more set-ups are ONE device
 * submission — one input copy, one memset, one voting launch, one tail launch, one copy back, whatever n_setups is
 * (get "bruteforce_submits" counts the submissions of the brute-force solve entries); items of one set-up, and every
 * call with vote_arith 2, go through mpe_solve_bruteforce_batch, one call per set-up that has items.
 * n == 0: MPE_OK.  item_setup == NULL only with n_setups == 1.  A set-up that no item names is legal.  MPE_ERR_ARG
 * before any device work: null pointers, a set-up index out of range, n_markers outside 1 .. MPE_MAX_MARKERS, n_det[i]
 * outside 0 .. MPE_MAX_DETECTIONS, a lock-step or streaming submission of the handle not collected yet. */
int mpe_solve_bruteforce_batch_setups(mpe_handle* h, const double* det_xy, const int* n_det, const int* item_setup, int n,
                                      const mpe_track_setup* setups, int n_setups, mpe_result* out, uint32_t* hist,
                                      uint32_t* corr);

/* ---- detection sets of 65 .. MPE_WIDE_DETECTIONS points (a glare frame: more than MPE_MAX_DETECTIONS blobs pass the
 * shape filter).  The reference has no limit (pose_estimator.cpp:549-557 votes for any image_points_.size()); the
 * ordinary entries refuse n_det > MPE_MAX_DETECTIONS.  A separate surface: no ordinary entry, record or status changes.
 * Row strides are MPE_WIDE_DETECTIONS here, and detection indices (1-based, up to 256) are uint32 throughout.
 *
 * mpe_vote_batch_wide ≙ mpe_vote_batch (initialise()'s loop nest, pose_estimator.cpp:565-702) for 0 .. MPE_WIDE_DETECTIONS
 * detections per set: det_xy n_frames x MPE_WIDE_DETECTIONS x 2, n_det[f] valid rows; hist n_frames x MPE_WIDE_DETECTIONS x
 * MPE_MAX_MARKERS.  Always the strict arithmetic (one block per 1024 hypotheses of a set, spread over the chip): with
 * vote_arith 3 / 4 the histograms of 4 / 3, with 1 / 0 those of 0 / 1 — for a set of up to MPE_MAX_DETECTIONS points the
 * rows mpe_vote_batch returns.  vote_arith 2 (the fast arithmetic alone) has no strict form: MPE_ERR_UNSUPPORTED.
 *
 * mpe_solve_bruteforce_batch_wide ≙ mpe_solve_bruteforce_batch (setImagePoints + initialise + optimiseAndUpdatePose,
 * pose_estimator.cpp:80-91,544-721,733-812): det_xy n x MPE_WIDE_DETECTIONS x 2; hist (optional) n x MPE_WIDE_DETECTIONS x
 * MPE_MAX_MARKERS; corr (optional) n x 2*MPE_MAX_MARKERS, rows (marker, detection) with the detection's index in the
 * caller's set (1 .. 256).  One submission for any n: one input copy, one memset, the wide voting launch, a small kernel
 * that runs the all-zero test (pose_estimator.cpp:704) and correspondencesFromHistogram (:344-370) and hands the at most
 * n_markers detections those rows name — all that checkCorrespondences and optimisePose read (:394-542, 733-792) — to
 * the validate / refine kernels of mpe_check_and_refine, one copy back.  Status and record as mpe_solve_bruteforce: 1
 * with the identity pose and zero covariance when the histogram is all zero, fewer than 4 detections or markers are
 * given or the rows are rejected; out[i].n_det = n_det[i].
 *
 * Both: n == 0: MPE_OK.  MPE_ERR_ARG before any device work: null pointers, n_det[i] outside 0 .. MPE_WIDE_DETECTIONS,
 * n_markers outside 1 .. MPE_MAX_MARKERS, a lock-step or streaming submission of the handle not collected yet.
 * get "wide_frames": detection sets of more than MPE_MAX_DETECTIONS points mpe_solve_bruteforce_batch_wide has solved
 * since the handle was made (see mpe_estimate_batch_wide).
 * set "wide_block_cap" (tests): blocks per set of the wide voting launch at most (0 = automatic, four per compute unit);
 * the histograms do not depend on it.
 *
 * mpe_detect_batch_wide ≙ mpe_detect_batch (LEDDetector::findLeds, led_detector.cpp:35-112, which loops over every
 * contour) with records of MPE_WIDE_DETECTIONS points: the image scan and the general blob tier (its LDS-resident kernel
 * with option "general_lds" 1) over every frame of the call — kept blobs and order (descending raster order of the
 * contour's start pixel) as that tier computes them for mpe_detect_batch, only the cut-off moves from 64 to 256.  A frame
 * that still exceeds a capacity keeps the code mpe_detect_batch gives it: a frame on which 257 blobs (or any number above
 * 256) pass the filter gets MPE_FRAME_TOO_MANY_DETECTIONS (-10) with n = 256 and the first 256 of the reference's order
 * (unless more than 512 passed: which blobs it then holds is unspecified, as for the narrow record); bright rows beyond
 * the band capacity: MPE_FRAME_TOO_MANY_ROWS (-12).  MPE_FRAME_TOO_MANY_BLOBS (-11) is not produced by this tier — it
 * counts the blobs that PASS, not the raw contours.
 *
 * mpe_estimate_batch_wide ≙ mpe_estimate_batch, arguments and all: it runs mpe_estimate_batch, then takes every frame
 * whose record says MPE_FRAME_TOO_MANY_DETECTIONS through mpe_detect_batch_wide (one call per such frame: they are rare)
 * and all of them through ONE mpe_solve_bruteforce_batch_wide, and overwrites those records; every other record is byte
 * for byte what mpe_estimate_batch wrote.  A frame beyond the wide capacities keeps its code.  Under vote_arith 2 the call
 * answers MPE_ERR_UNSUPPORTED only when a frame needs the wide solve (the records of mpe_estimate_batch are then in
 * `results`); a batch without such a frame is mpe_estimate_batch.  "wide_frames" counts the
 * frames solved this way (and, for direct callers of mpe_solve_bruteforce_batch_wide, the sets of more than
 * MPE_MAX_DETECTIONS points). */
int mpe_detect_batch_wide(mpe_handle* h, const uint8_t* frames, int n_frames, int rows, int cols, size_t stride_bytes,
                          size_t frame_stride_bytes, int frames_on_device, const double K[9], const double* D, int nD,
                          const mpe_params* p, mpe_detections_wide* dets);
int mpe_estimate_batch_wide(mpe_handle* h, const uint8_t* frames, int n_frames, int rows, int cols, size_t stride_bytes,
                            size_t frame_stride_bytes, int frames_on_device, const double* markers_xyz, int n_markers,
                            const double K[9], const double* D, int nD, const mpe_params* p, mpe_result* results);
int mpe_vote_batch_wide(mpe_handle* h, const double* det_xy, const int* n_det, int n_frames, const double* markers_xyz,
                        int n_markers, const double K[9], double back_projection_pixel_tolerance, uint32_t* hist);
int mpe_solve_bruteforce_batch_wide(mpe_handle* h, const double* det_xy, const int* n_det, int n,
                                    const double* markers_xyz, int n_markers, const double K[9], const mpe_params* p,
                                    mpe_result* out, uint32_t* hist, uint32_t* corr);

/* mpe_track_step_batch_wide ≙ mpe_track_step_batch_setups / _device / _device_encoded (the lock-step time step: ROI
 * detection, findCorrespondences from predicted_px, checkCorrespondences, optimisePose) with records of
 * MPE_WIDE_DETECTIONS points — a stream whose ROI fills with reflections.  Synchronous only: such steps are rare.
 * frames_on_device 0: items[i].img are host frames (mono8: encoding must be MPE_ENC_MONO8); 1: device frames in
 * `encoding` (MPE_ENC_*, stride_bytes in source bytes; src_big_endian for mono16).  item_setup == NULL only with
 * n_setups == 1.  One submission: the slots are packed / gathered as the narrow entries do it, then per set-up the image
 * scan, the general blob tier with the wide record, one small kernel (k_nn_wide: the nearest detection of every
 * predicted pixel, first minimum wins; the detections the rows name compacted into an ordinary record) and the
 * validation + refinement kernels; one copy back.  dets_out n records; corr_out n x 2*MPE_MAX_MARKERS words, rows
 * (marker, detection) 1-based with detection indices 1 .. 256; out[i].status 0 = refined, 1 = fewer than 4 LEDs, no
 * predicted_px (detection only) or rows rejected, < 0 = a capacity (more than 256 passing blobs: -10 with the first 256,
 * as mpe_detect_batch_wide answers).  For an item with at most MPE_MAX_DETECTIONS detections every record equals the
 * narrow entry's: n, status and the first n coordinates, the rows and n_corr, status, pose and covariance bit for bit
 * (the tail reads only the detections the rows name, in row order).  MPE_ERR_ARG / MPE_ERR_UNSUPPORTED before any
 * device work: the usage errors of the narrow entries, host frames with an encoding, a submission of the handle that is
 * not yet collected.  n == 0: MPE_OK.  get "wide_track_submits" counts the submissions of this entry. */
int mpe_track_step_batch_wide(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n, int rows, int cols,
                              size_t stride_bytes, int frames_on_device, int encoding, int src_big_endian,
                              const mpe_track_setup* setups, int n_setups, mpe_detections_wide* dets_out,
                              uint32_t* corr_out, mpe_result* out);

/* ---- stateful estimator: the whole PoseEstimator::estimateBodyPose state machine, i.e. the
 * uninitialised branch AND the tracking path (pose_estimator.cpp:62-147): pose prediction by the
 * constant-velocity model (predictPose :232-244), ROI from the predicted LED pixels
 * (LEDDetector::determineROI, led_detector.cpp:114-179), ROI detection with whole-image retry,
 * nearest-neighbour correspondences (findCorrespondences :372-392), validation + refinement,
 * fallback to brute-force initialisation (:831-848).  One tracker = one PoseEstimator object. */
typedef struct mpe_tracker mpe_tracker;
int mpe_tracker_create(mpe_handle* h, mpe_tracker** out);              /* PoseEstimator() */
void mpe_tracker_destroy(mpe_tracker* t);
int mpe_tracker_set_markers(mpe_tracker* t, const double* xyz, int n); /* setMarkerPositions */
int mpe_tracker_set_camera(mpe_tracker* t, const double K[9], const double* D, int nD);
int mpe_tracker_set_params(mpe_tracker* t, const mpe_params* p);       /* tuning members / setters */
int mpe_tracker_reset(mpe_tracker* t); /* back to "not initialised" (the reference has no reset) */
/* on != 0: a frame on which more than MPE_MAX_DETECTIONS blobs pass the shape filter — in the ROI of a tracked stream
 * or on the whole image of one that initialises — no longer ends with MPE_FRAME_TOO_MANY_DETECTIONS: the stream's
 * detection is repeated with the wide record (all such streams of a time step through ONE mpe_track_step_batch_wide),
 * and a brute force over more than MPE_MAX_DETECTIONS points goes through mpe_solve_bruteforce_batch_wide (one call per
 * set-up; at 256 detections / 5 markers it holds the handle for about 0.43 s, and a lock-step group waits for it).
 * The state machine is otherwise unchanged; getters and info[5] then report up to MPE_WIDE_DETECTIONS detections and
 * correspondence indices up to 256.  What keeps the -10 code: a frame with more than MPE_WIDE_DETECTIONS passing
 * blobs, and a wide brute force under vote_arith 2 (which has no strict form) — the other streams of the group get
 * their records.  Honoured by every entry that drives a tracker.  Default 0: nothing changes. */
int mpe_tracker_set_wide_frames(mpe_tracker* t, int on);
/* estimateBodyPose(image, time_to_predict): returns 1 pose updated, 0 not, <0 error.  out (optional)
 * gets getPredictedPose / getPoseCovariance; info (optional, 8 ints) = region_of_interest_
 * x,y,w,h, it_since_initialized_, detections, correspondences, 1 if brute force ran. */
int mpe_tracker_estimate(mpe_tracker* t, const uint8_t* img, int rows, int cols, size_t stride_bytes,
                         double time_to_predict, mpe_result* out, int info[8]);

/* estimateBodyPose for frame k of N trackers (N independent streams of the same camera model, marker set and
 * parameters, all created on the SAME handle) in lock step: the per-stream state machines run on the host as in
 * mpe_tracker_estimate, but every device step is ONE batched submission over the streams that need it
 * (mpe_track_step_batch for the ROI / whole-image detections with their validate + refine,
 * mpe_solve_bruteforce_batch for the re-initialisations): in steady state one submission per time step for all
 * N streams.  imgs[i], times[i]: stream i's frame and time stamp; out (optional) n records, info (optional)
 * n x 8 ints, updated (optional) n flags.  Results are identical to calling mpe_tracker_estimate per stream.
 * Returns the number of streams whose pose was updated, or <0 (usage / HIP error; a per-stream capacity overrun
 * is reported in out[i].status and that stream is left as its failed call leaves it). */
int mpe_tracker_estimate_batch(mpe_tracker* const* trackers, int n, const uint8_t* const* imgs, int rows, int cols,
                               size_t stride_bytes, const double* times, mpe_result* out, int* info, int* updated);

/* The image-callback loops of N streams in lock step over recorded sequences: frames[i] = stream i's sequence
 * (frame f at frames[i] + f*frame_stride_bytes), times[f] the common time stamps; out / info (optional):
 * n x n_frames records / n x n_frames x 8 ints, stream-major.  Returns the number of pose updates or <0.
 * The trackers may live on SEVERAL handles (same device or not): each handle's trackers form one lock-step group
 * (same camera / markers / parameters within a group), and the groups are pipelined against each other — while
 * the device works on step k of one group the host collects, advances and packs another — which hides the host
 * work of a time step behind the device latency.  Results do not depend on the grouping. */
int mpe_tracker_run_sequences_batch(mpe_tracker* const* trackers, int n, const uint8_t* const* frames, int n_frames,
                                    int rows, int cols, size_t stride_bytes, size_t frame_stride_bytes,
                                    const double* times, mpe_result* out, int* info);
/* The same with the groups spread over up to n_threads host threads (group g on thread g % n_threads; the groups of
 * one thread are pipelined against each other as above).  Groups share nothing — own handle and stream, own trackers,
 * own rows of out / info — so the records are those of the single-threaded call; with 64 streams in 4-8 groups the
 * host work of a time step no longer bounds the rate.  n_threads = 1: the call above. */
int mpe_tracker_run_sequences_batch_threads(mpe_tracker* const* trackers, int n, const uint8_t* const* frames,
                                            int n_frames, int rows, int cols, size_t stride_bytes,
                                            size_t frame_stride_bytes, const double* times, mpe_result* out, int* info,
                                            int n_threads);

/* mpe_tracker_estimate_batch for trackers that may differ in camera, marker set and parameters (one PoseEstimator per
 * camera: pose_estimator.h:63,82-83, monocular_pose_estimator.cpp:103-120).  The trackers must be distinct and on the
 * SAME handle (else MPE_ERR_ARG before any device work).  The ROI / whole-image detections of a time step go through
 * mpe_track_step_batch_setups — in steady state ONE device submission and one launch for all N streams —, the
 * re-initialisations of a step through ONE mpe_solve_bruteforce_batch_setups over the streams of every set-up that has
 * any (mpe_solve_bruteforce_batch when only one set-up has).  Results are identical to calling
 * mpe_tracker_estimate per stream, and to mpe_tracker_estimate_batch over each set-up's trackers alone. */
int mpe_tracker_estimate_batch_mixed(mpe_tracker* const* trackers, int n, const uint8_t* const* imgs, int rows, int cols,
                                     size_t stride_bytes, const double* times, mpe_result* out, int* info, int* updated);
/* mpe_tracker_run_sequences_batch_threads with groups formed by handle alone: each handle's trackers form one lock-step
 * group that may mix cameras, marker sets and parameters (as mpe_tracker_estimate_batch_mixed).  Same arguments, same
 * records as running each set-up's trackers as a uniform group. */
int mpe_tracker_run_sequences_batch_mixed_threads(mpe_tracker* const* trackers, int n, const uint8_t* const* frames,
                                                  int n_frames, int rows, int cols, size_t stride_bytes,
                                                  size_t frame_stride_bytes, const double* times, mpe_result* out,
                                                  int* info, int n_threads);

/* mpe_tracker_estimate_batch_mixed / mpe_tracker_run_sequences_batch_mixed_threads for frames in DEVICE memory:
 * d_imgs / d_frames are HOST arrays of device pointers (d_imgs[i] stream i's frame, d_frames[i] stream i's sequence),
 * on the device of the trackers' handle.  The ROI and whole-image detections go through
 * mpe_track_step_batch_setups_device_submit instead of the host-frame submission — no frame and no ROI crosses PCIe —,
 * the re-initialisations through mpe_solve_bruteforce_batch[_setups] on detections that are on the host anyway.  The trackers
 * may mix set-ups (the _mixed rules: distinct trackers, one handle per group).  Records and info are byte-identical to
 * those of the host-frame entries over the same frames.  Ordering as for mpe_track_step_batch_setups_device: the
 * frames are final in the order of the handle's stream at the call and unmodified until it returns. */
int mpe_tracker_estimate_batch_device(mpe_tracker* const* trackers, int n, const uint8_t* const* d_imgs, int rows,
                                      int cols, size_t stride_bytes, const double* times, mpe_result* out, int* info,
                                      int* updated);
int mpe_tracker_run_sequences_batch_device_threads(mpe_tracker* const* trackers, int n, const uint8_t* const* d_frames,
                                                   int n_frames, int rows, int cols, size_t stride_bytes,
                                                   size_t frame_stride_bytes, const double* times, mpe_result* out,
                                                   int* info, int n_threads);
/* The two entries above for device frames in the camera's own encoding (MPE_ENC_*, one value per call; src_big_endian
 * for MPE_ENC_MONO16; stride_bytes and frame_stride_bytes in SOURCE bytes, rows and cols in pixels): the detections go
 * through mpe_track_step_batch_setups_device_encoded_submit, the whole-image ones (a cold first step, a retry) as well —
 * the gather then decodes the whole frame.  Records and info are byte-identical to those of the entries above over
 * the same frames after mpe_convert_to_mono8.  An encoding outside MPE_ENC_* is MPE_ERR_UNSUPPORTED, a stride below
 * cols * bytes per pixel MPE_ERR_ARG, both before any tracker is touched. */
int mpe_tracker_estimate_batch_device_encoded(mpe_tracker* const* trackers, int n, const uint8_t* const* d_imgs, int rows,
                                              int cols, size_t stride_bytes, int encoding, int src_big_endian,
                                              const double* times, mpe_result* out, int* info, int* updated);
int mpe_tracker_run_sequences_batch_device_encoded_threads(mpe_tracker* const* trackers, int n,
                                                           const uint8_t* const* d_frames, int n_frames, int rows, int cols,
                                                           size_t stride_bytes, size_t frame_stride_bytes, int encoding,
                                                           int src_big_endian, const double* times, mpe_result* out,
                                                           int* info, int n_threads);

/* mpe_tracker_estimate_batch_mixed / mpe_tracker_run_sequences_batch_mixed_threads (frames_on_device 0: host frames,
 * every format MPE_ENC_MONO8) and their _device_encoded forms (frames_on_device 1) for trackers whose cameras differ in
 * image format as well: formats[i] is stream i's (mpe_image_format above), frame_stride_bytes[i] its sequence stride in
 * source bytes.  The _mixed rules hold — distinct trackers, one handle per group, for _threads the groups by handle,
 * pipelined as before.  Whole-image ROI, determineROI, the size class and the whole-image retry of a stream use that
 * stream's rows and cols; the detections of a time step go through ONE mpe_track_step_batch_formats_submit (equal
 * formats once in its table), the rare wide re-detections through one mpe_track_step_batch_wide per distinct format
 * among those streams, the re-initialisations through the brute-force entries as before (they work on detections).
 * Results are identical to mpe_tracker_estimate per stream and to the entries above over each format's trackers alone.
 * A null pointer, a bad format (rows, cols, stride) or an encoded format with host frames is MPE_ERR_ARG, an encoding
 * outside MPE_ENC_* MPE_ERR_UNSUPPORTED, all before any tracker is touched. */
int mpe_tracker_estimate_batch_formats(mpe_tracker* const* trackers, int n, const uint8_t* const* imgs, int frames_on_device,
                                       const mpe_image_format* formats, const double* times, mpe_result* out, int* info,
                                       int* updated);
int mpe_tracker_run_sequences_batch_formats_threads(mpe_tracker* const* trackers, int n, const uint8_t* const* frames,
                                                    int n_frames, int frames_on_device, const mpe_image_format* formats,
                                                    const size_t* frame_stride_bytes, const double* times, mpe_result* out,
                                                    int* info, int n_threads);

/* The estimator's private state (pose_estimator.h:56-62, 74-79), for callers that drive the public
 * step methods of the class (predictPose, findCorrespondences, ... — see compat/) between calls of
 * mpe_tracker_estimate.  Poses row-major 4x4. */
typedef struct mpe_tracker_state {
  double current_pose[16], previous_pose[16], predicted_pose[16];
  double pose_covariance[36];
  double current_time, previous_time, predicted_time;
  unsigned it_since_initialized;
  int roi[4]; /* region_of_interest_ x, y, width, height */
} mpe_tracker_state;
int mpe_tracker_get_state(const mpe_tracker* t, mpe_tracker_state* st);
int mpe_tracker_set_state(mpe_tracker* t, const mpe_tracker_state* st);

/* Host arithmetic of the state machine, exported so that the facade and the tracker share ONE
 * implementation (no device involved): predictPose (pose_estimator.cpp:232-244: constant-velocity
 * extrapolation through logarithmMap / exponentialMap), exponentialMap (:962-994), logarithmMap
 * (:996-1064), project2d for a list of marker positions (:251-276; markers n x 3, px n x 2). */
int mpe_predict_pose(const double current_pose[16], const double previous_pose[16], double current_time,
                     double previous_time, double time_to_predict, double predicted_pose[16]);
int mpe_exponential_map(const double twist[6], double T[16]);
int mpe_logarithm_map(const double T[16], double twist[6]);
int mpe_project_points(const double T[16], const double* markers_xyz, int n, const double K[9], double* px);
/* findCorrespondences (pose_estimator.cpp:372-392): corr gets up to n_markers rows (marker, detection),
 * 1-based; returns the number of rows (>= 0) or MPE_ERR_ARG. */
int mpe_find_correspondences(const double* predicted_px, int n_markers, const double* det_xy, int n_det,
                             double nearest_neighbour_pixel_tolerance, uint32_t* corr);

/* The image callback loop (MPENode::imageCallback -> estimateBodyPose, monocular_pose_estimator.cpp:
 * 125-190) over a recorded sequence: frame f at frames + f*frame_stride_bytes with time stamp
 * times[f].  out (optional) n_frames records, info (optional) n_frames x 8 ints as above.  Returns
 * the number of frames whose pose was updated, or <0 on the first usage / HIP error.  A frame that exceeds
 * a device capacity (MPE_FRAME_TOO_MANY_*) does not end the sequence: its record is zeroed, out[f].status
 * holds the code, the estimator state is as that frame's failed call left it, and the replay continues. */
int mpe_tracker_run_sequence(mpe_tracker* t, const uint8_t* frames, int n_frames, int rows, int cols,
                             size_t stride_bytes, size_t frame_stride_bytes, const double* times,
                             mpe_result* out, int* info);

/* getCorrespondences() / getImagePoints() of the tracker object: copy up to cap rows / points,
 * return the number available (or <0). */
int mpe_tracker_get_correspondences(mpe_tracker* t, uint32_t* corr, int cap_rows);
int mpe_tracker_get_image_points(mpe_tracker* t, double* xy, int cap_points);
/* distorted_detection_centers_ of the last detection (what the overlay circles, pose_estimator.cpp:44-48) */
int mpe_tracker_get_distorted_centers(mpe_tracker* t, float* xy, int cap_points);

/* ---- several cameras, one body: the cameras of a calibrated rig fused into ONE pose (joint Gauss-Newton) ----
 * A rig has 1 .. MPE_RIG_MAX_CAMERAS cameras; camera c has K_c and a rigid extrinsic T_cam_rig = E_c = [R_c | t_c],
 * camera <- rig, row-major 4x4 (trusted: the upper 3x4 is used as it is, orthonormality is not checked).  The unknown
 * is T, rig <- marker frame.  The refinement is PoseEstimator::optimisePose (pose_estimator.cpp:733-792) over rows
 * (camera, marker xyz, undistorted pixel uv) that bring their own camera: per row q = E_c T p, the residual and the
 * closed-form Jacobian of computeJacobian (:945-957) at q with K_c, times the 6x6 adjoint of E_c (twist order
 * (upsilon, omega)); A = sum J^T J and b = sum J^T e in row order, unpivoted LDL^T, T <- exp(dT) T, stop at
 * max|dT| <= 1e-13 or after 500 iterations, cov = A^-1 of the last iteration: the covariance of a left twist in the RIG
 * frame.  One camera with the identity extrinsic gives mpe_optimise_pose's pose, covariance and count, bit for bit. */
#define MPE_RIG_MAX_CAMERAS 16
typedef struct mpe_rig_camera {
  double K[9];
  double T_cam_rig[16];
} mpe_rig_camera;

/* Stage entry: n_problems problems over ONE rig; the rows of problem i are [row_begin[i], row_begin[i+1]) of
 * row_camera / row_marker_xyz (x 3) / row_uv (x 2), at most MPE_RIG_MAX_CAMERAS * MPE_MAX_MARKERS = 256 of them, in
 * summation order (camera after camera, each in its correspondence order).  T_init: n x 16; out: n HOST records —
 * T (rig <- marker), cov, gn_iterations, n_corr = rows used, n_det = cameras that contributed a row, status
 * MPE_FRAME_POSE, or MPE_FRAME_NO_POSE with fewer than 3 rows (T = T_init, cov = 0) or a non-finite final pose.  Rank
 * deficiency beyond that is the caller's concern, as in the reference.  One input copy, one launch (a wave per
 * problem; a problem's record does not depend on the rest of the batch) and one copy back on the handle's stream.
 * MPE_ERR_ARG: a null pointer, n_cameras outside 1 .. 16, a camera index outside the rig, a decreasing row_begin, a
 * submission of the handle that is not collected yet; MPE_ERR_UNSUPPORTED: more than 256 rows in a problem; no record
 * is written then.  n_problems == 0: MPE_OK, nothing submitted. */
int mpe_rig_optimise_pose_batch(mpe_handle* h, const mpe_rig_camera* cameras, int n_cameras, const int* row_begin,
                                const int* row_camera, const double* row_marker_xyz, const double* row_uv,
                                int n_problems, const double* T_init, mpe_result* out);

/* After a lock-step call over the n trackers of a rig (one per camera, all on one handle, one marker set = one body):
 * fuse those whose frame updated (updated[i] != 0; NULL = all).  Tracker i brings its K, its markers and the rows of
 * its last correspondences over its image points (mpe_tracker_get_correspondences / _get_image_points), T_cam_rig
 * (n x 16) its extrinsic; the start is E_c^-1 * pose_c of the first contributing tracker.  One problem through
 * mpe_rig_optimise_pose_batch.  rows_per_camera (optional, n ints).  Returns 1 fused (rig_out->status MPE_FRAME_POSE),
 * 0 no pose (no tracker contributed, or the status above), MPE_ERR_ARG before any device work for trackers on
 * different handles, repeated trackers, differing marker sets, or n outside 1 .. 16. */
int mpe_rig_fuse_trackers(mpe_tracker* const* trackers, int n, const double* T_cam_rig, const int* updated,
                          mpe_result* rig_out, int* rows_per_camera);

/* Give trackers a pose from the rig — host state only (what mpe_tracker_get_state / _set_state move).  For every i with
 * seed[i] != 0: current_pose = predicted_pose = E_i * rig_pose, current_time = time; with rig_prev_pose also
 * previous_pose = E_i * rig_prev_pose, previous_time = prev_time and it_since_initialized = 2 (the next frame predicts
 * with the constant-velocity model), without it it_since_initialized = 1.  Covariance and ROI are left alone.  The next
 * frame of such a tracker takes the reference's tracking branch (predictWithROI, nearest neighbour, validation, fallback
 * to initialise() as ever) instead of the brute force. */
int mpe_rig_seed_trackers(mpe_tracker* const* trackers, int n, const double* T_cam_rig, const int* seed,
                          const double rig_pose[16], double time, const double* rig_prev_pose, double prev_time);

/* ---- tracking a body with the whole rig: a camera that sees fewer than four LEDs counts ----
 * mpe_rig_fuse_trackers takes rows only from cameras whose own tracker solved the frame (>= 4 LEDs in that camera).  The
 * step below needs no camera to stand on its own: from a predicted rig pose T_pred (rig <- marker frame) it matches every
 * camera's detections to the projected markers and refines ONE pose over all rows.  A problem = one time step of one
 * rig; round r = 0, 1, .. starts from T_r (T_0 = T_pred):
 *  1. project: q = E_c T_r p_m, (u, v) as mpe_rig_optimise_pose_batch computes them; visible when q_z > 0 and u, v finite;
 *  2. match: the nearest detection of camera c (findCorrespondences' arithmetic: du*du + dv*dv, strict <, first minimum
 *     wins), kept when sqrt(best) <= tol_c — match_tolerance[c] in round 0, accept_tolerance[c] in later rounds;
 *  3. one marker per detection: of several markers of a camera on one detection the smallest squared distance keeps it,
 *     a tie goes to the lowest marker index; the others get no row this round (no second-nearest search);
 *  4. rows in ascending (camera, marker) order; fewer than min_rows: no pose, reason 1; fewer than min_markers distinct
 *     markers among them: no pose, reason 2;
 *  5. r > 0 and the row set equals the previous round's: stop, the result is the previous round's refinement;
 *  6. refine: mpe_rig_optimise_pose_batch's iteration from T_r over the rows -> T_{r+1}; a non-finite pose: no pose,
 *     reason 3; stop when r + 1 == max_rounds.
 * Accept: at the final pose every final row's residual length must be <= accept_tolerance[c], else no pose, reason 4.
 * This rule is the project's own: the reference validates correspondences with a P3P triple inside ONE camera
 * (checkCorrespondences), which a camera with two or three rows cannot supply.  It is no initialiser: it needs T_pred.
 * A record without a pose (status MPE_FRAME_NO_POSE) has T = T_pred and cov = 0; info and match_out still say what was
 * computed (the last row set built).  With a pose: T, cov (left twist in the rig frame) and gn_iterations are those of
 * the last refinement, n_corr = rows, n_det = cameras with a row.  info: rounds = refinements run, rows /
 * distinct_markers of the last row set, reason 0 .. 4, max_residual / rms (pixels) of the accept test (0 when it was not
 * reached). */
typedef struct mpe_rig_track_options {
  int max_rounds;  /* 2; 1 .. 4 */
  int min_rows;    /* 4; >= 3 */
  int min_markers; /* 3; >= 1 */
} mpe_rig_track_options;
void mpe_rig_track_default_options(mpe_rig_track_options* o);
typedef struct mpe_rig_track_info {
  int rounds, rows, distinct_markers, reason;
  double max_residual, rms;
} mpe_rig_track_info;
/* n_problems problems over ONE rig and ONE marker set (markers_xyz n_markers x 3).  The detections (undistorted
 * pixels) of camera c in problem i are the points [det_begin[i * n_cameras + c], det_begin[i * n_cameras + c + 1]) of
 * det_xy (x 2), at most MPE_MAX_DETECTIONS of them; det_begin has n_problems * n_cameras + 1 entries.  match_tolerance /
 * accept_tolerance: n_cameras each, > 0 (+inf allowed).  T_pred: n x 16.  options == NULL: the defaults.  out: n HOST
 * records; match_out (optional): n_problems * n_cameras * n_markers words, the 1-based detection within that camera's
 * list that gave (camera, marker) its row, 0 = none; info_out (optional): n records.  One input copy, one launch (a
 * wave per problem; a problem's record does not depend on the rest of the batch) and one copy back on the handle's
 * stream.  MPE_ERR_ARG before any device work: a null pointer, n_cameras or n_markers outside 1 .. 16, a negative or
 * decreasing det_begin, an option out of range, a tolerance that is not > 0, a submission of the handle that is not
 * collected yet; MPE_ERR_UNSUPPORTED: a camera list of more than MPE_MAX_DETECTIONS detections; nothing is written then.
 * n_problems == 0: MPE_OK, nothing submitted. */
int mpe_rig_track_batch(mpe_handle* h, const mpe_rig_camera* cameras, int n_cameras, const double* markers_xyz,
                        int n_markers, const int* det_begin, const double* det_xy, const double* match_tolerance,
                        const double* accept_tolerance, int n_problems, const double* T_pred,
                        const mpe_rig_track_options* options, mpe_result* out, uint32_t* match_out,
                        mpe_rig_track_info* info_out);

/* After a lock-step call over the n trackers of a rig: ONE problem through mpe_rig_track_batch from rig_pred_pose (rig <-
 * marker frame at this frame's time).  Tracker i brings its K, the shared marker set and ALL its image points of that
 * frame (mpe_tracker_get_image_points), whether or not the frame gave that camera a pose; its
 * nearest_neighbour_pixel_tolerance is the match tolerance and its back_projection_pixel_tolerance the accept tolerance.
 * (The image points of a camera whose ROI held fewer than four LEDs are those of its whole-image retry; when the retry
 * found nothing, those of the ROI.)  rig_out: the record; match_out (optional) n x n_markers words; info_out (optional).
 * Tracker state is not touched.  Returns 1 pose, 0 none, and refuses what mpe_rig_fuse_trackers refuses (MPE_ERR_ARG
 * before any device work); a tracker with more than MPE_MAX_DETECTIONS image points: MPE_ERR_UNSUPPORTED. */
int mpe_rig_track_trackers(mpe_tracker* const* trackers, int n, const double* T_cam_rig, const double rig_pred_pose[16],
                           const mpe_rig_track_options* options, mpe_result* rig_out, uint32_t* match_out,
                           mpe_rig_track_info* info_out);

/* ---- finding a body with the whole rig: no camera needs four LEDs, one needs three ----
 * The tracking step above keeps a pose; this step gets one.  It is initialise() (pose_estimator.cpp:544-702: a P3P
 * hypothesis from every detection triple x marker permutation, scored by reprojection) widened from one camera to the
 * rig: hypotheses come from every camera with at least three detections, support is counted in ALL cameras.  A problem =
 * one time step of one rig: the cameras, one marker set, per camera a list of undistorted detections, a vote tolerance
 * and an accept tolerance.
 *  Items.  The cameras in ascending order; camera c with n_c >= 3 detections brings every detection triple i < j < k in
 *   lexicographic order, crossed with every ordered triple of distinct markers in lexicographic order: item = offset of
 *   the camera + rank of the combination * P(n_markers, 3) + rank of the permutation.  Bearings as calculateImageVectors,
 *   the P3P of the voting entries (Kneip; Ferrari's quartic in plain double arithmetic) per root 0 .. 3; a solution
 *   counts when it is finite.  Hypothesis h = 4 * item + root, T_h = E_c^-1 [R^T | -R^T C] (rig <- marker frame), both
 *   rigid inverses in closed form.
 *  Score.  Steps 1 - 3 of mpe_rig_track_batch at T_h, in that entry's arithmetic, with the vote tolerance: the row set
 *   W_h, rows_h = |W_h|, s2_h = the kept squared distances summed in ascending (camera, marker) order.
 *  Winner.  The least key (rows descending, s2 ascending, h ascending), a total order: the result cannot depend on how
 *   the hypotheses were spread over the device.
 *  Runner-up.  runner_rows = the largest rows_h among the hypotheses that CONTRADICT the winner — some (c, m) has a row in
 *   W_h that is not the winner's row for (c, m) —, 0 when there is none.
 *  Decision, in this order: no finite hypothesis: reason 6; best_rows < min_rows: reason 1; fewer than min_markers
 *   distinct markers in the winner's rows: reason 2; best_rows - runner_rows < min_margin: reason 5 (ambiguous); else the
 *   tracking rounds of mpe_rig_track_batch from T_pred = T_winner with match tolerance = vote tolerance, the accept
 *   tolerance, max_rounds, min_rows and min_markers: their reasons (1 .. 4) pass through; reason 0: pose, covariance,
 *   iterations and counts are the tracking step's.
 * A record without a pose has T = I, cov = 0 and status MPE_FRAME_NO_POSE.
 * This acceptance rule is this library's own, like the tracking step's: the reference validates a hypothesis inside the
 * one camera that produced it, with a fourth LED of that camera, and such a camera does not exist here.  The defaults
 * come from a numpy prototype (5 markers, 0.1 px noise, 2 stray detections per camera, 3 px tolerance): with the LEDs
 * spread [3, 3, 2] over three cameras the true row set won with 8 rows while contradicting hypotheses reached 5 - 7; with
 * [3, 2, 1] or [3, 2, 2], or with clutter alone, wrong hypotheses of 4 - 6 rows appeared that the residual test of the
 * tracking rounds accepted — hence min_rows above the tracking step's 4 and the strict margin.  Both guards turn a true
 * problem with few rows into "no pose" (INTEGRATION.md gives the shares); a caller with a tighter tolerance may lower
 * them.  One camera with three blobs is needed: a rig in which every camera sees at most two has no hypothesis. */
typedef struct mpe_rig_init_options {
  int max_rounds;  /* 2; 1 .. 4 */
  int min_rows;    /* 6; >= 3 */
  int min_markers; /* 4; >= 1 */
  int min_margin;  /* 1; >= 0, 0 switches the margin test off */
} mpe_rig_init_options;
void mpe_rig_init_default_options(mpe_rig_init_options* o);
typedef struct mpe_rig_init_info {
  int reason;                   /* 0 pose; 1 .. 4 as mpe_rig_track_info; 5 ambiguous; 6 no finite hypothesis;
                                   7 (mpe_rig_init_bodies_batch only) the body was not asked for */
  int camera;                   /* the winner: its camera (-1 without a winner), */
  int detection[3], marker[3];  /*  detection triple (0-based within the camera's list) and marker triple, */
  int root;                     /*  and root */
  int best_rows, runner_rows;
  int best_markers;             /* distinct markers among the winner's rows */
  int64_t n_items;              /* purely combinatorial: sum over the cameras of C(n_c, 3) * P(n_markers, 3) */
  double best_sum2;
  double T_hyp[16];             /* T_winner (I without a winner) */
  mpe_rig_track_info track;     /* the tracking rounds' (zero when they did not run) */
} mpe_rig_init_info;
/* n_problems problems over ONE rig and ONE marker set, laid out as mpe_rig_track_batch's (det_begin, det_xy, the two
 * tolerance arrays, out, match_out, info_out).  match_out: the tracking rounds' when they ran, else the winner's row set.
 * One input copy, four launches on the handle's stream (vote, winner, runner-up, finish) and one copy back; a problem's
 * record does not depend on the rest of the batch.  Refusals as mpe_rig_track_batch's (min_margin < 0: MPE_ERR_ARG), and
 * MPE_ERR_UNSUPPORTED before any device work for a problem of more than 2^22 items (admitted: 16 cameras x 12 detections x
 * 8 markers = 1.18 M items, 3 cameras x 20 detections x 8 markers = 1.15 M, one list of 64 with 5 markers = 2.5 M;
 * not: one list of 64 with 6 markers = 5.0 M); nothing is written then.  get "rig_init_submits" counts submissions. */
int mpe_rig_init_batch(mpe_handle* h, const mpe_rig_camera* cameras, int n_cameras, const double* markers_xyz,
                       int n_markers, const int* det_begin, const double* det_xy, const double* vote_tolerance,
                       const double* accept_tolerance, int n_problems, const mpe_rig_init_options* options,
                       mpe_result* out, uint32_t* match_out, mpe_rig_init_info* info_out);

/* After a lock-step call over the n trackers of a rig: ONE problem through mpe_rig_init_batch.  Tracker i brings its K,
 * the shared marker set and ALL its image points of that frame; its back_projection_pixel_tolerance is both the vote and
 * the accept tolerance (initialise() votes with that tolerance too).  Tracker state is not touched.  Returns 1 pose, 0
 * none, and refuses what mpe_rig_fuse_trackers refuses. */
int mpe_rig_init_trackers(mpe_tracker* const* trackers, int n, const double* T_cam_rig, const mpe_rig_init_options* options,
                          mpe_result* rig_out, uint32_t* match_out, mpe_rig_init_info* info_out);

/* ---- several bodies in one frame: rounds of the rig initialiser, each in what the earlier ones left ----
 * Every other entry assumes ONE body in view.  Here a problem is still one time step of one rig of 1 ..
 * MPE_RIG_MAX_CAMERAS cameras, with the detection lists and the two tolerance arrays laid out as mpe_rig_init_batch's,
 * but instead of one marker set there are n_bodies bodies, 1 .. MPE_MAX_BODIES; body b has its own markers and its own
 * options, and two bodies may have the same marker set.
 *  claimed_in (optional): one byte per point of det_xy, same indexing; non-zero: the detection is available to no body.
 *  find (optional): n_problems x n_bodies flags, problem-major; NULL: every body is searched.
 *  Rounds b = 0 .. n_bodies - 1, in this order, per problem.  The FREE LIST of camera c is its detections that are not
 *   claimed — by claimed_in or by an earlier round —, in ascending index order.
 *  find[i][b] == 0: the record has status MPE_FRAME_NO_POSE, T = I, cov = 0 and zero counts, the info record is zeroed
 *   with reason 7 (not asked), the match words are 0, nothing is claimed.
 *  Otherwise the record, the info and the match words of (i, b) are what mpe_rig_init_batch returns for the free lists
 *   with body b's markers and options, byte for byte, except for the indices that name detections: the match words are
 *   1-based indices within the CALLER's list of that camera and info.detection[3] is 0-based within the caller's list of
 *   that camera.  info.n_items is the count over the free lists.
 *  Claim.  When the record has a pose (reason 0), every detection a non-zero match word of this round names is claimed by
 *   b.  A round without a pose claims nothing.
 *  owner_out (optional): one int8_t per point of det_xy: -1 free, -2 claimed at entry, else the body that claimed it.
 * Layouts: out and info_out n_problems x n_bodies records, problem-major; match_out per (problem, body) n_cameras x
 * MPE_MAX_MARKERS words (a fixed stride, the bodies differ in marker count; the words behind a body's n_markers are 0).
 * A problem's records do not depend on the rest of the batch.
 * The acceptance rule is the rig initialiser's above, which is this library's own; for several bodies the reference has
 * no counterpart at all (its PoseEstimator is one body: initialise() sums the votes of all hypotheses into one histogram,
 * and two bodies in view vote into the same rows).
 * The bodies' defaults (options == NULL; mpe_rig_init_bodies_default_options): max_rounds 2; min_margin 0 — an identical
 * second body always contradicts the winner with equal rows, so the margin test cannot be kept —; with one camera
 * min_rows = min_markers = n_markers (a single camera can never reach 6 rows of 5 markers), with two or more min_rows 6
 * and min_markers 4 as mpe_rig_init_default_options.  INTEGRATION.md says what they were checked on.
 * One submission per call whatever n_bodies is: one input copy, per round the peel step (the claims of the round before,
 * the free lists compacted on the device) and the initialiser's four launches, one copy back, one synchronise; no host
 * round trip between rounds.  get "rig_init_bodies_submits" counts the submissions; "rig_init_submits" does not move.
 * Refusals, all before any device work: those of mpe_rig_init_batch, per body; n_bodies outside 1 .. MPE_MAX_BODIES:
 * MPE_ERR_ARG; a body that is asked for whose item count over the lists left by claimed_in exceeds 2^22:
 * MPE_ERR_UNSUPPORTED (later rounds only shrink the lists); a submission of the handle not collected yet.  n_problems == 0
 * returns MPE_OK. */
#define MPE_MAX_BODIES 16
typedef struct mpe_rig_body {
  const double* markers_xyz;
  int n_markers;
  const mpe_rig_init_options* options; /* NULL: the bodies' defaults */
} mpe_rig_body;
void mpe_rig_init_bodies_default_options(mpe_rig_init_options* o, int n_cameras, int n_markers);
int mpe_rig_init_bodies_batch(mpe_handle* h, const mpe_rig_camera* cameras, int n_cameras, const mpe_rig_body* bodies,
                              int n_bodies, const int* det_begin, const double* det_xy, const uint8_t* claimed_in,
                              const uint8_t* find, const double* vote_tolerance, const double* accept_tolerance,
                              int n_problems, mpe_result* out, uint32_t* match_out, mpe_rig_init_info* info_out,
                              int8_t* owner_out);

/* After a lock-step call over n_bodies x n_cameras trackers, body-major (tracker [b][c] = trackers[b * n_cameras + c] is
 * body b in camera c; all on one handle): ONE problem through mpe_rig_init_bodies_batch for the bodies with find[b] != 0
 * (find NULL: all).  Camera c's list is the image points of tracker [b0][c], b0 the lowest body that is asked for — the
 * points mpe_rig_init_trackers takes; the note on mpe_rig_track_trackers about the whole-image retry applies: a tracker
 * that was not tracking detects in the whole image, one that lost its body in its ROI brings the ROI's points when the
 * retry found none.  That tracker's back_projection_pixel_tolerance is the vote and the accept tolerance; body b's
 * markers are its trackers'; every body runs with the bodies' defaults.  For n_cameras == 1 T_cam_rig may be NULL: the
 * identity.
 * Claims at entry come from the bodies that are being tracked: for every [b][c] with find[b] == 0 and updated[b *
 * n_cameras + c] != 0 (updated NULL: all), each image point a correspondence row of that tracker names claims every
 * point q of camera c's list with dx * dx + dy * dy <= claim_radius_px^2 (host, plain double).  The radius is there
 * because a tracked body's points come from the detection in its ROI and the list from a whole-image detection, whose
 * blobs may differ in the last digits; 0 claims exact coordinates only.
 * rig_out / info_out: n_bodies records; match_out: n_bodies x n_cameras x MPE_MAX_MARKERS words; owner_out (optional): a
 * byte per point of the lists, camera after camera.  Tracker state is not touched: seed the found bodies with
 * mpe_rig_seed_trackers.  Returns the number of bodies that got a pose (find all zero: 0 = MPE_OK, nothing submitted,
 * every record "not asked"), or < 0: what mpe_rig_fuse_trackers refuses, per body; n_bodies outside 1 ..
 * MPE_MAX_BODIES; trackers of one camera that differ in K or in the distortion coefficients; a negative or non-finite radius; what the batch entry
 * refuses. */
int mpe_rig_init_bodies_trackers(mpe_tracker* const* trackers, int n_bodies, int n_cameras, const double* T_cam_rig,
                                 const int* find, const int* updated, double claim_radius_px, mpe_result* rig_out,
                                 uint32_t* match_out, mpe_rig_init_info* info_out, int8_t* owner_out);

/* ---- calibrating the extrinsics of a rig from the body it tracks (a bundle adjustment on the device) ----
 * A recorded sequence of ONE body in front of the rig: view f (a time step) holds the rows [view_begin[f],
 * view_begin[f+1]) of row_camera / row_marker_xyz (x 3) / row_uv (x 2, undistorted pixels), in any camera order, at most
 * 256 of them.  The unknowns are a left twist on the pose T_f (rig <- marker frame) of every used view and a left twist
 * on the extrinsic E_c (camera <- rig) of every camera but reference_camera, which keeps its extrinsic (the gauge); the
 * residual is mpe_rig_optimise_pose_batch's, e = uv - project(K_c, E_c T_f p).  Plain Gauss-Newton with a Schur
 * complement over the view poses, unpivoted LDL^T, every sum in row order / view order by one lane (no atomics: the
 * same bits from run to run); stop when the largest |component| of all twists of an iteration is <= step_tolerance, or
 * after max_iterations.
 * Which rows take part: a view is used when it has >= 3 rows of >= 2 distinct cameras and its cameras are linked to the
 * reference camera through such views; a camera that is not (or has no rows) is HELD — its extrinsic comes back as
 * given, its rows are dropped; the poses of unused views come back as given.  Rank deficiency beyond these rules is the
 * caller's concern.
 * cameras: K and the START extrinsics; T_view_init: n_views x 16 start poses (mpe_rig_calibration_start makes both from
 * per-camera poses).  T_cam_rig_out: n_cameras x 16; T_view_out (optional): n_views x 16; cov_out (optional): n_cameras
 * x 36, the 6 x 6 diagonal block of the inverse of the reduced system of the last iteration — the marginal covariance
 * of the camera's left twist for unit pixel noise, zero for the reference camera and held cameras; view_used
 * (optional): n_views flags; report: status MPE_FRAME_POSE / MPE_FRAME_NO_POSE, iterations, views and rows used,
 * rms = sqrt(mean e^2) over the residual components of the used rows at the start values and at the final values,
 * last_step, camera_state (0 reference, 1 calibrated, 2 held) and camera_rows (rows used) per camera.
 * Returns 1 calibrated; 0 not (no used view, or a non-finite output: status MPE_FRAME_NO_POSE, every extrinsic and view
 * pose comes back as given, cov_out zero); before any device work MPE_ERR_ARG (a null pointer, n_cameras outside 1 ..
 * 16, n_views < 0, a camera index outside the rig, a negative or decreasing view_begin, reference_camera outside the
 * rig, max_iterations < 1, step_tolerance not positive, a submission of the handle that is not collected yet) or
 * MPE_ERR_UNSUPPORTED (a view of more than 256 rows).  options == NULL: the defaults.  Any number of views per call:
 * the views' records are worked through in chunks (set "rig_ba_record_kb": their device buffer at most, 0 = 65536).
 * set "rig_ba_profile" 1: every launch of a call is bracketed by events; get "rig_ba_us_linearise" / "_reduce" /
 * "_solve" / "_update" / "_finish" / "_covariance" (device time of the last call per step, microseconds) and
 * "rig_ba_launches". */
typedef struct mpe_rig_calibration_options {
  int reference_camera; /* 0 */
  int max_iterations;   /* 50 */
  double step_tolerance; /* 1e-10 */
} mpe_rig_calibration_options;
void mpe_rig_calibration_default_options(mpe_rig_calibration_options* o);
typedef struct mpe_rig_calibration_report {
  int status, iterations, views_used, rows_used;
  double rms_before, rms_after, last_step;
  int camera_state[MPE_RIG_MAX_CAMERAS], camera_rows[MPE_RIG_MAX_CAMERAS];
} mpe_rig_calibration_report;
int mpe_rig_calibrate(mpe_handle* h, const mpe_rig_camera* cameras, int n_cameras, const int* view_begin,
                      const int* row_camera, const double* row_marker_xyz, const double* row_uv, int n_views,
                      const double* T_view_init, const mpe_rig_calibration_options* options, double* T_cam_rig_out,
                      double* T_view_out, double* cov_out, int* view_used, mpe_rig_calibration_report* report);

/* Start values for mpe_rig_calibrate from per-camera poses (what a lock-step call returns) — host only.  camera_pose:
 * n_views x n_cameras x 16, camera <- marker frame; updated: n_views x n_cameras flags (a pose counts when non-zero).
 * E_ref = I; breadth first from reference_camera over the views in order, camera c is linked through the first view in
 * which c and an already linked c' both updated: E_c = P_cf P_c'f^-1 E_c' (an unlinked camera gets the identity,
 * camera_linked[c] = 0).  T_f = E_c^-1 P_cf of the lowest linked camera that updated in f, the identity if none did.
 * T_cam_rig_out: n_cameras x 16; T_view_out: n_views x 16; camera_linked (optional): n_cameras.  Returns the number of
 * linked cameras (the reference camera included), or MPE_ERR_ARG. */
int mpe_rig_calibration_start(const double* camera_pose, const int* updated, int n_views, int n_cameras,
                              int reference_camera, double* T_cam_rig_out, double* T_view_out, int* camera_linked);

/* ---- calibrating the LED positions of a body from the sequences it was tracked in (a bundle adjustment on the device) ----
 * Every other entry takes markers_xyz as exact; here they are the unknowns.  A recorded sequence of ONE body in front of
 * 1 .. MPE_RIG_MAX_CAMERAS cameras: cameras bring K and the extrinsic E_c (camera <- rig), which is trusted and stays
 * fixed (a single camera passes the identity).  View f holds the rows [view_begin[f], view_begin[f+1]) of row_camera /
 * row_marker / row_uv (x 2, undistorted pixels), in any order, at most 256 of them; row_marker is an INDEX into
 * markers_xyz (n_markers x 3, 1 .. MPE_MAX_MARKERS: the START positions).  T_view_init: n_views x 16 start poses, rig <-
 * marker frame.  The unknowns are a left twist on the pose T_f of every used view and an additive delta_m on every FREE
 * marker; the residual is mpe_rig_optimise_pose_batch's, e = uv - project(K_c, E_c T_f p_m).  Plain Gauss-Newton with a
 * Schur complement over the view poses, unpivoted LDL^T, every sum in row / view / marker order by one lane (no atomics:
 * the same bits from run to run); stop when the largest |component| of all twists and deltas of an iteration is <=
 * step_tolerance, or after max_iterations.
 * Which rows take part — a fixed point that starts with every marker free: a view is used when its rows on free markers
 * number >= 4 and name >= 3 distinct free markers; a marker is free when it has >= 2 rows in used views.  A marker that
 * is not free is HELD: its position comes back as given, bit for bit, its rows are dropped; the poses of unused views
 * come back as given.  Fewer than 3 free markers or no used view: nothing is calibrated.  Rank deficiency beyond these
 * rules (too few views, collinear free markers, no motion) is the caller's concern, as for optimisePose.
 * The gauge: the body frame is arbitrary (6 degrees of freedom), and when no used view has used rows of two cameras the
 * size is unobservable too (a seventh).  They are fixed by inner constraints: with c the centroid of the free markers'
 * current positions and d_m = p_m - c, every step delta satisfies sum delta_m = 0, sum d_m x delta_m = 0 and, when scale
 * is held, sum d_m . delta_m = 0 — the result is the shape the data give, placed (and, with scale held, sized) where the
 * start values were, to first order.  scale: -1 held exactly when no used view has used rows of two cameras, 0 free, 1
 * held; report.scale_held says which.
 * markers_out: n_markers x 3; T_view_out (optional): n_views x 16; cov_out (optional): n_markers x 9, the 3 x 3 diagonal
 * block of the pseudo-inverse of the reduced system of the last iteration — the inner-constraint covariance of the
 * marker for unit pixel noise, zero for a held marker (scale = 1 on a rig that observes the size: the covariance of
 * the estimate under that constraint, and every step is the constrained one); view_used (optional): n_views flags; report: status, iterations,
 * views / rows used, markers_free, scale_held, rms = sqrt(mean e^2) over the used rows at the start and the final
 * values, last_step, marker_state (1 calibrated, 2 held) and marker_rows (rows used) per marker.
 * Returns 1 calibrated; 0 not (the rules above, or a non-finite output: status MPE_FRAME_NO_POSE, markers and poses come
 * back exactly as given, cov_out zero); before any device work MPE_ERR_ARG (a null pointer, n_cameras outside 1 .. 16,
 * n_markers outside 1 .. 16, n_views < 0, a camera or marker index out of range, a negative or decreasing view_begin,
 * scale outside -1 .. 1, max_iterations < 1, step_tolerance not positive, a submission of the handle that is not
 * collected yet) or MPE_ERR_UNSUPPORTED (a view of more than 256 rows); nothing is written then.  options == NULL: the
 * defaults.  The views' records are worked through in chunks under "rig_ba_record_kb", as mpe_rig_calibrate's.  set
 * "rig_ba_profile" 1: get "body_ba_us_linearise" / "_reduce" / "_solve" / "_update" / "_finish" / "_covariance" (device
 * time of the last call per step, microseconds) and "body_ba_launches".
 * The acceptance rules and the gauge are this library's own: the reference has no such step. */
typedef struct mpe_body_calibration_options {
  int scale;             /* -1 */
  int max_iterations;    /* 50 */
  double step_tolerance; /* 1e-10 */
} mpe_body_calibration_options;
void mpe_body_calibration_default_options(mpe_body_calibration_options* o);
typedef struct mpe_body_calibration_report {
  int status, iterations, views_used, rows_used, markers_free, scale_held;
  double rms_before, rms_after, last_step;
  int marker_state[MPE_MAX_MARKERS], marker_rows[MPE_MAX_MARKERS];
} mpe_body_calibration_report;
int mpe_body_calibrate(mpe_handle* h, const mpe_rig_camera* cameras, int n_cameras, const double* markers_xyz,
                       int n_markers, const int* view_begin, const int* row_camera, const int* row_marker,
                       const double* row_uv, int n_views, const double* T_view_init,
                       const mpe_body_calibration_options* options, double* markers_out, double* T_view_out,
                       double* cov_out, int* view_used, mpe_body_calibration_report* report);

/* Stage-level batch entry points (used by the parity tests at every stage boundary). */
/* detection only (a1): dets is a HOST array of n_frames records */
int mpe_detect_batch(mpe_handle* h, const uint8_t* frames, int n_frames, int rows, int cols,
                     size_t stride_bytes, size_t frame_stride_bytes, int frames_on_device,
                     const double K[9], const double* D, int nD, const mpe_params* p,
                     mpe_detections* dets);
/* voting only (a4, PE.cpp:544-702): det_xy is n_frames x MPE_MAX_DETECTIONS x 2 (host), n_det[f]
 * valid rows each; hist is n_frames x MPE_MAX_DETECTIONS x MPE_MAX_MARKERS (host) */
int mpe_vote_batch(mpe_handle* h, const double* det_xy, const int* n_det, int n_frames,
                   const double* markers_xyz, int n_markers, const double K[9],
                   double back_projection_pixel_tolerance, uint32_t* hist);

/* Forensics for the parity soaks (tests/forensics.py): the voting of mpe_vote_batch restricted, per detection set, to
 * the hypotheses [item_lo[f], item_hi[f]) of initialise()'s loop nest — flattened index = detection-triple index x
 * P(n_markers,3) + marker-permutation index, both in the reference's table order (combinations.cpp:52-203,
 * pose_estimator.cpp:565-600).  With n copies of one detection set and ranges [i, i+1) it returns every hypothesis'
 * own votes, which is how a HIP-vs-oracle histogram difference is traced to the hypotheses that cast it.  Same
 * kernels and arithmetic as mpe_vote_batch (option "vote_arith" applies). */
int mpe_vote_items(mpe_handle* h, const double* det_xy, const int* n_det, int n_frames, const double* markers_xyz,
                   int n_markers, const double K[9], double back_projection_pixel_tolerance, const int* item_lo,
                   const int* item_hi, uint32_t* hist);

/* Time (ms) of the kernels of the last mpe_estimate_batch* call, measured with HIP events on the
 * handle's stream: [0] image scan, [1] blob extraction, [2] voting, [3] validate+refine, [4] total.
 * Only valid after mpe_set_profiling(h, 1); profiling adds event records to the stream. */
int mpe_set_profiling(mpe_handle* h, int enable);
int mpe_last_kernel_ms(mpe_handle* h, float ms[5]);
/* A large batch runs as several sub-batches (option "pipeline"): every kernel is then launched once
 * per sub-batch and mpe_last_kernel_ms reports the AVERAGE PER LAUNCH.  This returns the number of
 * launches per kernel and the frames each one processed for the last profiled call. */
/* Same for ONE sub-batch of a pipelined call (0 <= sub_batch < launches): scan, blobs, vote, tail.  With
 * pipeline_mode 3 ("fused") the scan of sub-batch s + 1 runs INSIDE the voting kernel of sub-batch s: the
 * vote time of every sub-batch but the last then includes that scan, and scan = the stand-alone scan
 * launches only (the whole first sub-batch, afterwards only remainders of less than one chunk). */
int mpe_last_kernel_ms_sub(mpe_handle* h, int sub_batch, float ms[4]);
int mpe_last_launch_shape(mpe_handle* h, int* launches, int* frames_per_launch);

/* Tuning knobs that are not part of the reference surface: "lds_budget" (bytes of LDS per frame
 * for the blob bitmaps, 8192..163840), "vote_splits" (workgroups per frame in the voting kernel,
 * 0 = auto), "pipeline" (a large call is cut into up to this many sub-batches of about 32768 frames — 16384 for frames larger than 512 KB —,
 * default 16, 1 = one chain of four kernels), "pipeline_mode" (how the sub-batches are scheduled:
 * -1 automatic (default) = 6;  0 = two-stream software
 * pipeline, the scan of sub-batch s+1 beside the voting of sub-batch s;  3 = fused, one stream: the
 * scan of sub-batch s+1 rides inside the voting kernel of sub-batch s;  4 = as 3, with the validate /
 * refine kernels of sub-batch s on an internal side stream, beside the blob extraction of sub-batch
 * s+1 (joined back before the call returns its place on the stream);  6 = as 4, and the image scan of a
 * sub-batch is split: "scan_split_pct" % of it (default 30) is taken by a stand-alone scan kernel on a second
 * side stream during the blob / tail window two sub-batches earlier ("side_scan_blocks" resident blocks per CU,
 * default 3), the voting kernel's rider scans the rest), "k1a_dummy_lds" (occupancy cap
 * of the stand-alone scan kernel in mode 0, per handle), "ingest_chunk" (frames per chunk of the double-buffered
 * host-frame ingest of mpe_estimate_batch, default 2048, 0 = one blocking copy per call), "refine_variant" (the refinement kernel: 0 automatic = 16 lanes per frame for launches of up to 2048 frames, else one lane per frame; 1 / 2 force one of them; bit-identical results), "vote_arith" (arithmetic of the voting kernel:
 * 3 (default since round 6) = fast — Newton-Raphson division / square root, Newton cube root, per-permutation
 * tables, [R|C]-free back-projection — with every hypothesis it cannot decide safely re-evaluated by the strict
 * functions, whose quartic evaluates std::pow(complex, double) of p3p.cpp:262,264,268 as libstdc++ / glibc do
 * (exp(y log|z|) through clog's branches; csrc/mpe_ddmath.h): the vote histograms of the CPU reference build also in
 * the unstable corner of its Ferrari solver; 1 = the same with exact products / cbrt(hypot)
 * for those powers (default of rounds 4 - 5); 4 / 0 = strict — the validation kernel's P3P functions with IEEE
 * operators in the reference's statement order for every hypothesis, powers as in 3 / 1; slower, never fused with
 * the scan; 2 = the fast arithmetic alone (A/B measurements).  3 and 4 produce identical histograms, as do 1 and 0.
 * Results are bit-identical in every pipeline mode (for a given vote_arith). */
int mpe_set_option(mpe_handle* h, const char* name, int value);
/* Measurement read-outs through the same pair of calls:
 * set "vote_events" = N > 0: a pair of timing events is recorded around every voting launch that carries a scan, for
 *   the launches of the last N pipelined calls — nothing else, so a timed region stays what it is; get
 *   "vote_launch_ns_mean" / "vote_launches" (synchronises the handle's stream); set 0 to release the events.
 * set "track_profile" = 1 starts / resets host-side timers of every tracked submission (mpe_track_step, the lock-step
 *   batch entries and the tracker entries on top of them); get "track_ns_pack" (to the input copy issued),
 *   "track_ns_enqueue" (to the last command queued), "track_ns_wait" (to the records in hand in _collect; mean ns per
 *   step), "track_steps" (submissions collected).
 * get "track_batch_submits", "track_batch_chains", "track_batch_reruns": device submissions of the tracked entries
 *   (mpe_track_step, mpe_track_step_batch[_setups][_submit], and every tracker entry on top of them, a lone tracker's
 *   mpe_tracker_estimate / mpe_tracker_run_sequence included), set-ups of a submission
 *   that ran through the chain of kernels instead of the one fused launch (track_fused 0, more than 8 markers), and
 *   set-ups repeated through that chain by _collect because a slot overflowed the small blob tier; since the handle was
 *   made.
 * get "bruteforce_submits": device submissions of the brute-force solve entries since the handle was made
 *   (mpe_solve_bruteforce, mpe_initialise, mpe_solve_bruteforce_batch: one per call; mpe_solve_bruteforce_batch_setups:
 *   one for a call that goes out fused, else one per set-up that has items; the trackers' re-initialisations included).
 * get "overflow_frames", "overflow_general", "overflow_why_1" .. "overflow_why_6": frames of the last pipelined batch
 *   that the first blob tier handed on, in all / to the general tier / by the capacity exceeded (bright segments,
 *   bands, islands, pixel pool, bitmap pool, blobs kept); synchronises.
 * get "vote_fixup_items" / "vote_fixup_overflow" / "vote_relost_frames": hypotheses the fast voting kernel handed to
 *   the strict arithmetic since the handle was made, appends that found their list full, and frames that were therefore
 *   voted again by the strict loop nest (a full list costs time, never a pose); synchronises.
 * Tuning / test knobs (round 5): "vote_list_cap" (entries per suspect list at most, 0 = no limit: a tiny list exercises
 *   the re-vote path), "k1b_general_blocks" (PROCESS-wide: blocks = scratch slabs of the general blob tier, 32 .. 8192,
 *   default 4096, within 1 GB of scratch, never more than the frames of a launch nor than the blocks the device holds
 *   at once — 4 096 on an MI355X: a block walks the work-list with the grid as its stride), "tail_priority" /
 *   "scan_priority" (stream priority of the library's two side streams, applied when they are created: -1 lowest,
 *   0 ordinary streams, 1 highest, 2 the default level but created through the priority entry point; default 1 / 1 —
 *   off the default level so that they get hardware queues of their own, DESIGN.md section 3, Schedules.  NOTE for
 *   callers: at 1 the side streams' kernels are dispatched ahead of work on the caller's own ordinary-priority
 *   streams of the same process while a pipelined call is in flight; set both to -1 to keep the queues and yield
 *   instead — same step time within noise, profiles/round5_exp_side_priorities.json).
 * "detections_hint" (round 6): detections per frame the caller expects in device-resident / streaming calls (0 =
 *   automatic: the number of markers, or what the last call whose records came back to the host saw — read-out
 *   "detections_seen").  From 9 on the <= 5-marker voting kernel prefilters its back-projections with an occupancy
 *   grid of the detections instead of a distance per detection; the suspect lists are sized from it.  Results do not
 *   depend on it.
 * "track_fused" (round 6): 2 (default) a tracked frame / lock-step time step is ONE launch (k_track_frame) that also
 *   stores the records to pinned host memory; 1 the same with a copy command for the records; 0 the chain of four
 *   kernels + two copies of rounds 3 - 5.  Bit-identical records.  "track_phase_clocks" = 1: that kernel stamps its
 *   phases; get "track_phase_cycles_0" .. "_3" (scan, blobs, validation, refinement: mean shader-clock cycles).
 * "general_lds" (round 6): kernel of the general blob tier — 0 (default) bitmaps in global-memory slabs, 16 frames per
 *   CU in flight, (band, column run, row piece) items of any number per frame for frames up to 3 966 pixels wide; 1 a
 *   block per CU with the frame's bitmaps in LDS (faster per frame, one frame per CU: 2 x slower on
 *   salt noise, 7 % faster on one large blob); -1 the LDS kernel once the previous call saw frames reach the tier
 *   (read-out "general_seen").  Bit-identical detections.
 * get "vote_wide_frames" (round 6): frames with more than MPE_FAST_VOTE_DETECTIONS detections, voted by the strict
 *   loop nest alone; synchronises. */
/* Read an option back.  Also "streams_concurrent": 1 once the library has verified (spin-kernel probe at
 * the first large batch) that its two pipeline side streams execute concurrently, 0 if no concurrent
 * pair was found (the runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues), -1 not probed yet;
 * "last_schedule": the pipeline_mode the last large batch actually ran with. */
int mpe_get_option(mpe_handle* h, const char* name, int* value);

/* library / device introspection */
int mpe_device_count(void);
const char* mpe_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MPE_H_ */
