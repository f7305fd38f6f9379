// mpe_rig.cpp — host side of libmpe_hip.so, part 6 (see mpe_host.h): the cameras of a calibrated rig fused into one body
// pose.  mpe_rig_optimise_pose_batch — the joint Gauss-Newton (k_rig_refine, mpe_k3.hip; logic in mpe_rig_gn.h) over
// rows that bring their own camera: one input copy, one launch, one copy back.  What works on the trackers of a rig
// (mpe_rig_fuse_trackers, mpe_rig_seed_trackers) is in mpe_tracker.cpp, beside the state it reads and sets, and comes
// here through the public entry.
#include "mpe_host.h"

namespace {
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
}  // namespace

extern "C" {

int mpe_rig_optimise_pose_batch(mpe_handle* h, const mpe_rig_camera* cameras, int n_cameras, const int* row_begin,
                                const int* row_camera, const double* row_marker_xyz, const double* row_uv,
                                int n_problems, const double* T_init, mpe_result* out) {
  if (!h || n_problems < 0) return fail(h, MPE_ERR_ARG, "bad argument");
  if (!cameras) return fail(h, MPE_ERR_ARG, "cameras is null");
  if (!row_begin) return fail(h, MPE_ERR_ARG, "row_begin is null");
  if (!T_init) return fail(h, MPE_ERR_ARG, "T_init is null");
  if (!out) return fail(h, MPE_ERR_ARG, "out is null");
  if (n_cameras < 1 || n_cameras > MPE_RIG_MAX_CAMERAS) return fail(h, MPE_ERR_ARG, "n_cameras outside 1 .. MPE_RIG_MAX_CAMERAS");
  if (n_problems == 0) return MPE_OK;
  if (row_begin[0] < 0) return fail(h, MPE_ERR_ARG, "row_begin is negative");
  for (int i = 0; i < n_problems; ++i) {
    if (row_begin[i + 1] < row_begin[i]) return fail(h, MPE_ERR_ARG, "row_begin decreases");
    if (row_begin[i + 1] - row_begin[i] > MPE_RIG_MAX_CAMERAS * MPE_MAX_MARKERS)
      return fail(h, MPE_ERR_UNSUPPORTED, "more than MPE_RIG_MAX_CAMERAS * MPE_MAX_MARKERS rows in a problem");
  }
  const int r0 = row_begin[0], n_rows = row_begin[n_problems] - r0;
  if (n_rows > 0 && (!row_camera || !row_marker_xyz || !row_uv)) return fail(h, MPE_ERR_ARG, "a row array is null");
  for (int j = 0; j < n_rows; ++j)
    if (row_camera[r0 + j] < 0 || row_camera[r0 + j] >= n_cameras) return fail(h, MPE_ERR_ARG, "camera index outside the rig");
  if (h->pending_track_n || h->submit_seq != h->collect_seq)
    return fail(h, MPE_ERR_ARG, "a submitted batch has not been collected yet");
  ENTER(h);
  // in: [cameras | row_begin (rebased to 0) | row cameras | marker xyz | pixels | start poses]; back: the records
  const size_t cam_bytes = (size_t)n_cameras * sizeof(mpe_rig_camera);
  const size_t beg_off = up256(cam_bytes);
  const size_t rc_off = beg_off + up256((size_t)(n_problems + 1) * sizeof(int));
  const size_t xyz_off = rc_off + up256((size_t)n_rows * sizeof(int));
  const size_t uv_off = xyz_off + up256((size_t)n_rows * 3 * sizeof(double));
  const size_t t_off = uv_off + up256((size_t)n_rows * 2 * sizeof(double));
  const size_t in_bytes = t_off + (size_t)n_problems * 16 * sizeof(double);
  const size_t back_off = up256(in_bytes), back_bytes = (size_t)n_problems * sizeof(mpe_result);
  { const int rc = grow_mailbox(h, back_off + back_bytes); if (rc != MPE_OK) return rc; }
  uint8_t* mb = static_cast<uint8_t*>(h->mailbox);
  std::memcpy(mb, cameras, cam_bytes);
  int* hb = reinterpret_cast<int*>(mb + beg_off);
  for (int i = 0; i <= n_problems; ++i) hb[i] = row_begin[i] - r0;
  if (n_rows > 0) {
    std::memcpy(mb + rc_off, row_camera + r0, (size_t)n_rows * sizeof(int));
    std::memcpy(mb + xyz_off, row_marker_xyz + (size_t)3 * r0, (size_t)n_rows * 3 * sizeof(double));
    std::memcpy(mb + uv_off, row_uv + (size_t)2 * r0, (size_t)n_rows * 2 * sizeof(double));
  }
  std::memcpy(mb + t_off, T_init, (size_t)n_problems * 16 * sizeof(double));
  HIP_TRY(h, h->frames.reserve(in_bytes));
  HIP_TRY(h, h->results.reserve(back_bytes));
  uint8_t* d_in = static_cast<uint8_t*>(h->frames.p);
  mpe_result* d_res = static_cast<mpe_result*>(h->results.p);
  HIP_TRY(h, hipMemcpyAsync(d_in, mb, in_bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, launch_k_rig_refine(reinterpret_cast<const mpe_rig_camera*>(d_in), n_cameras,
                                 reinterpret_cast<const int*>(d_in + beg_off), reinterpret_cast<const int*>(d_in + rc_off),
                                 reinterpret_cast<const double*>(d_in + xyz_off), reinterpret_cast<const double*>(d_in + uv_off),
                                 reinterpret_cast<const double*>(d_in + t_off), n_problems, d_res, h->stream));
  HIP_TRY(h, hipMemcpyAsync(mb + back_off, d_res, back_bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  std::memcpy(out, mb + back_off, back_bytes);
  return MPE_OK;
}

}  // extern "C"
