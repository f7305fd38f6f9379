// mpe_rig.cpp — host side of libmpe_hip.so, part 6 (see mpe_host.h): the cameras of a calibrated rig fused into one body
// pose.  mpe_rig_optimise_pose_batch — the joint Gauss-Newton (k_rig_refine, mpe_k3.hip; logic in mpe_rig_gn.h) over
// rows that bring their own camera: one input copy, one launch, one copy back.  mpe_rig_track_batch — the partial-view
// tracking step (k_rig_track; logic in mpe_rig_track.h), submitted the same way.  mpe_rig_init_batch — the body found
// with the whole rig (k_rig_init_vote / _winner / _finish; logic in mpe_rig_init.h): the host counts the items and the
// voting blocks of every problem, one input copy, four launches, one copy back.  mpe_rig_init_bodies_batch — several bodies
// in one frame: that chain once per body over the detections the earlier bodies left, the peel step of mpe_rig_peel.hip
// (logic in mpe_rig_peel.h) between the rounds, still one input copy and one copy back.  What works on the trackers of a rig
// (mpe_rig_fuse_trackers, mpe_rig_track_trackers, mpe_rig_init_trackers, mpe_rig_seed_trackers) is in mpe_tracker.cpp, beside the state it reads and sets, and comes
// here through the public entry.  mpe_rig_calibrate — the extrinsics of a rig from a recorded sequence of the body: which
// rows take part and the iteration are mpe_rig_ba_plan.h (shared with the CPU tier), the steps are the k_rig_ba_* kernels
// (mpe_k3.hip; logic in mpe_rig_ba.h), one launch each on the handle's stream; the host reads two doubles per iteration.
// mpe_rig_calibration_start — start values from per-camera poses, host only.  mpe_body_calibrate — the LED positions of
// the body from such a sequence, the extrinsics fixed: the same iteration over the k_body_ba_* kernels (logic in
// mpe_body_ba.h), the row rules in mpe_body_ba_plan.h.
#include "mpe_host.h"
#include "mpe_rig_ba_plan.h"
#include "mpe_body_ba_plan.h"

namespace {
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the steps of rig_ba_iterate as launches on the handle's stream: Dev / Launch are the extrinsic calibration's (RigBaDev,
// launch_k_rig_ba) or the marker calibration's (BodyBaDev, launch_k_body_ba); ms / launches: where the handle keeps the
// profile of that entry
template <class Dev, hipError_t (*Launch)(int, const Dev&, int, int, int, hipStream_t)>
struct BaLaunches {
  mpe_handle* h;
  Dev d;
  double* ms;
  int* launches;
  double* host_out;  // pinned: where finish's two doubles land
  hipError_t err = hipSuccess;
  struct Timed {
    int step;
    hipEvent_t a, b;
  };
  std::vector<Timed> timed;  // option "rig_ba_profile": a pair of events around every launch
  int run(int step, int first, int count, int flag) {
    Timed t = {step, nullptr, nullptr};
    const bool prof = h->rig_ba_profile != 0;
    if (prof) {  // (whatever was created is in `timed` before anything can fail: read_out gives it back)
      if ((err = hipEventCreate(&t.a)) == hipSuccess) err = hipEventCreate(&t.b);
      timed.push_back(t);
      if (err != hipSuccess || (err = hipEventRecord(t.a, h->stream)) != hipSuccess) return 1;
    }
    err = Launch(step, d, first, count, flag, h->stream);
    if (prof && err == hipSuccess) err = hipEventRecord(t.b, h->stream);
    return err == hipSuccess ? 0 : 1;
  }
  // behind the last synchronisation of the call: the sums per step into the handle, the events given back
  void read_out() {
    if (!timed.empty()) {
      for (int k = 0; k < 6; ++k) ms[k] = 0;
      *launches = (int)timed.size();
    }
    for (const Timed& t : timed) {
      float el = 0;
      if (t.a && t.b && hipEventElapsedTime(&el, t.a, t.b) == hipSuccess) ms[t.step] += el;
      if (t.a) (void)hipEventDestroy(t.a);
      if (t.b) (void)hipEventDestroy(t.b);
    }
    timed.clear();
  }
  ~BaLaunches() { read_out(); }
  int linearise(int first, int count) { return run(MPE_RIG_BA_LINEARISE, first, count, 0); }
  int reduce(int first, int count, bool restart) { return run(MPE_RIG_BA_REDUCE, first, count, restart ? 1 : 0); }
  int solve() { return run(MPE_RIG_BA_SOLVE, 0, 0, 0); }
  int update(int first, int count) { return run(MPE_RIG_BA_UPDATE, first, count, 0); }
  int covariance() { return run(MPE_RIG_BA_COVARIANCE, 0, 0, 0); }
  int finish(int apply, double out2[2]) {
    if (run(MPE_RIG_BA_FINISH, 0, 0, apply)) return 1;
    if ((err = hipMemcpyAsync(host_out, d.out, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream)) != hipSuccess) return 1;
    if ((err = hipStreamSynchronize(h->stream)) != hipSuccess) return 1;
    out2[0] = host_out[0];
    out2[1] = host_out[1];
    return 0;
  }
};

// option "rig_launch_profile": a pair of events around the ONE launch of a batch entry.  begin() in front of the launch,
// end() behind it (both enqueue only), read() behind the call's synchronisation; the events are given back in any case.
struct RigLaunchTimer {
  mpe_handle* h;
  hipEvent_t a = nullptr, b = nullptr;
  explicit RigLaunchTimer(mpe_handle* h_) : h(h_) {}
  hipError_t begin() {
    if (!h->rig_launch_profile) return hipSuccess;
    hipError_t e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    if (e == hipSuccess) e = hipEventRecord(a, h->stream);
    return e;
  }
  hipError_t end() { return (a && b) ? hipEventRecord(b, h->stream) : hipSuccess; }
  void read() {
    float ms = 0;
    if (a && b && hipEventElapsedTime(&ms, a, b) == hipSuccess) h->rig_launch_ms = ms;
  }
  ~RigLaunchTimer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

struct M44 {
  double a[16];
};
M44 m44_from(const double* p) {
  M44 m;
  std::memcpy(m.a, p, sizeof(m.a));
  return m;
}
M44 m44_identity() {
  M44 m = {};
  for (int i = 0; i < 16; i += 5) m.a[i] = 1.0;
  return m;
}
M44 m44_mul(const M44& x, const M44& y) {
  M44 r;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = 0;
      for (int k = 0; k < 4; ++k) s += x.a[4 * i + k] * y.a[4 * k + j];
      r.a[4 * i + j] = s;
    }
  return r;
}
M44 m44_rigid_inverse(const M44& x) {  // [R | t]^-1 = [R^T | -R^T t]
  M44 r = m44_identity();
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) r.a[4 * i + j] = x.a[4 * j + i];
    r.a[4 * i + 3] = -(x.a[i] * x.a[3] + x.a[4 + i] * x.a[7] + x.a[8 + i] * x.a[11]);
  }
  return r;
}
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
  RigLaunchTimer timer(h);
  HIP_TRY(h, timer.begin());
  HIP_TRY(h, launch_k_rig_refine(reinterpret_cast<const mpe_rig_camera*>(d_in), n_cameras,
                                 reinterpret_cast<const int*>(d_in + beg_off), reinterpret_cast<const int*>(d_in + rc_off),
                                 reinterpret_cast<const double*>(d_in + xyz_off), reinterpret_cast<const double*>(d_in + uv_off),
                                 reinterpret_cast<const double*>(d_in + t_off), n_problems, d_res, h->stream));
  HIP_TRY(h, timer.end());
  HIP_TRY(h, hipMemcpyAsync(mb + back_off, d_res, back_bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  timer.read();
  std::memcpy(out, mb + back_off, back_bytes);
  return MPE_OK;
}

void mpe_rig_track_default_options(mpe_rig_track_options* o) {
  if (!o) return;
  o->max_rounds = 2;
  o->min_rows = 4;
  o->min_markers = 3;
}

int mpe_rig_track_batch(mpe_handle* h, const mpe_rig_camera* cameras, int n_cameras, const double* markers_xyz,
                        int n_markers, const int* det_begin, const double* det_xy, const double* match_tolerance,
                        const double* accept_tolerance, int n_problems, const double* T_pred,
                        const mpe_rig_track_options* options, mpe_result* out, uint32_t* match_out,
                        mpe_rig_track_info* info_out) {
  if (!h || n_problems < 0) return fail(h, MPE_ERR_ARG, "bad argument");
  if (!cameras) return fail(h, MPE_ERR_ARG, "cameras is null");
  if (!markers_xyz) return fail(h, MPE_ERR_ARG, "markers_xyz is null");
  if (!det_begin) return fail(h, MPE_ERR_ARG, "det_begin is null");
  if (!match_tolerance || !accept_tolerance) return fail(h, MPE_ERR_ARG, "a tolerance array is null");
  if (!T_pred) return fail(h, MPE_ERR_ARG, "T_pred is null");
  if (!out) return fail(h, MPE_ERR_ARG, "out is null");
  if (n_cameras < 1 || n_cameras > MPE_RIG_MAX_CAMERAS) return fail(h, MPE_ERR_ARG, "n_cameras outside 1 .. MPE_RIG_MAX_CAMERAS");
  if (n_markers < 1 || n_markers > MPE_MAX_MARKERS) return fail(h, MPE_ERR_ARG, "n_markers outside 1 .. MPE_MAX_MARKERS");
  mpe_rig_track_options opt;
  mpe_rig_track_default_options(&opt);
  if (options) opt = *options;
  if (opt.max_rounds < 1 || opt.max_rounds > 4) return fail(h, MPE_ERR_ARG, "max_rounds outside 1 .. 4");
  if (opt.min_rows < 3) return fail(h, MPE_ERR_ARG, "min_rows must be >= 3");
  if (opt.min_markers < 1) return fail(h, MPE_ERR_ARG, "min_markers must be >= 1");
  for (int c = 0; c < n_cameras; ++c)
    if (!(match_tolerance[c] > 0) || !(accept_tolerance[c] > 0)) return fail(h, MPE_ERR_ARG, "a tolerance is not > 0");
  if (n_problems == 0) return MPE_OK;
  const size_t n_lists = (size_t)n_problems * (size_t)n_cameras;
  if (det_begin[0] < 0) return fail(h, MPE_ERR_ARG, "det_begin is negative");
  for (size_t i = 0; i < n_lists; ++i)
    if (det_begin[i + 1] < det_begin[i]) return fail(h, MPE_ERR_ARG, "det_begin decreases");
  for (size_t i = 0; i < n_lists; ++i)
    if (det_begin[i + 1] - det_begin[i] > MPE_MAX_DETECTIONS)
      return fail(h, MPE_ERR_UNSUPPORTED, "more than MPE_MAX_DETECTIONS detections in a camera's list");
  const int d0 = det_begin[0], n_det = det_begin[n_lists] - d0;
  if (n_det > 0 && !det_xy) return fail(h, MPE_ERR_ARG, "det_xy is null");
  if (h->pending_track_n || h->submit_seq != h->collect_seq)
    return fail(h, MPE_ERR_ARG, "a submitted batch has not been collected yet");
  ENTER(h);
  // in: [cameras | markers | match tolerances | accept tolerances | det_begin (rebased to 0) | detections | predicted
  // poses]; back: [records | match words | info records]
  const size_t cam_bytes = (size_t)n_cameras * sizeof(mpe_rig_camera);
  const size_t mk_off = up256(cam_bytes);
  const size_t tm_off = mk_off + up256((size_t)n_markers * 3 * sizeof(double));
  const size_t ta_off = tm_off + up256((size_t)n_cameras * sizeof(double));
  const size_t beg_off = ta_off + up256((size_t)n_cameras * sizeof(double));
  const size_t det_off = beg_off + up256((n_lists + 1) * sizeof(int));
  const size_t t_off = det_off + up256((size_t)n_det * 2 * sizeof(double));
  const size_t in_bytes = t_off + (size_t)n_problems * 16 * sizeof(double);
  const size_t rec_bytes = (size_t)n_problems * sizeof(mpe_result);
  const size_t match_words = n_lists * (size_t)n_markers;
  const size_t m_off = up256(rec_bytes);
  const size_t i_off = m_off + up256(match_words * sizeof(uint32_t));
  const size_t back_bytes = i_off + (size_t)n_problems * sizeof(mpe_rig_track_info);
  const size_t back_off = up256(in_bytes);
  { const int rc = grow_mailbox(h, back_off + back_bytes); if (rc != MPE_OK) return rc; }
  uint8_t* mb = static_cast<uint8_t*>(h->mailbox);
  std::memcpy(mb, cameras, cam_bytes);
  std::memcpy(mb + mk_off, markers_xyz, (size_t)n_markers * 3 * sizeof(double));
  std::memcpy(mb + tm_off, match_tolerance, (size_t)n_cameras * sizeof(double));
  std::memcpy(mb + ta_off, accept_tolerance, (size_t)n_cameras * sizeof(double));
  int* hb = reinterpret_cast<int*>(mb + beg_off);
  for (size_t i = 0; i <= n_lists; ++i) hb[i] = det_begin[i] - d0;
  if (n_det > 0) std::memcpy(mb + det_off, det_xy + (size_t)2 * d0, (size_t)n_det * 2 * sizeof(double));
  std::memcpy(mb + t_off, T_pred, (size_t)n_problems * 16 * sizeof(double));
  HIP_TRY(h, h->frames.reserve(in_bytes));
  HIP_TRY(h, h->results.reserve(back_bytes));
  uint8_t* d_in = static_cast<uint8_t*>(h->frames.p);
  uint8_t* d_back = static_cast<uint8_t*>(h->results.p);
  HIP_TRY(h, hipMemcpyAsync(d_in, mb, in_bytes, hipMemcpyHostToDevice, h->stream));
  RigLaunchTimer timer(h);
  HIP_TRY(h, timer.begin());
  HIP_TRY(h, launch_k_rig_track(reinterpret_cast<const mpe_rig_camera*>(d_in), n_cameras,
                                reinterpret_cast<const double*>(d_in + mk_off), n_markers,
                                reinterpret_cast<const int*>(d_in + beg_off), reinterpret_cast<const double*>(d_in + det_off),
                                reinterpret_cast<const double*>(d_in + tm_off), reinterpret_cast<const double*>(d_in + ta_off),
                                reinterpret_cast<const double*>(d_in + t_off), opt.max_rounds, opt.min_rows, opt.min_markers,
                                n_problems, reinterpret_cast<mpe_result*>(d_back),
                                reinterpret_cast<uint32_t*>(d_back + m_off),
                                reinterpret_cast<mpe_rig_track_info*>(d_back + i_off), h->stream));
  HIP_TRY(h, timer.end());
  HIP_TRY(h, hipMemcpyAsync(mb + back_off, d_back, back_bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  timer.read();
  std::memcpy(out, mb + back_off, rec_bytes);
  if (match_out) std::memcpy(match_out, mb + back_off + m_off, match_words * sizeof(uint32_t));
  if (info_out) std::memcpy(info_out, mb + back_off + i_off, (size_t)n_problems * sizeof(mpe_rig_track_info));
  return MPE_OK;
}

void mpe_rig_init_default_options(mpe_rig_init_options* o) {
  if (!o) return;
  o->max_rounds = 2;
  o->min_rows = 6;
  o->min_markers = 4;
  o->min_margin = 1;
}

int mpe_rig_init_batch(mpe_handle* h, const mpe_rig_camera* cameras, int n_cameras, const double* markers_xyz,
                       int n_markers, const int* det_begin, const double* det_xy, const double* vote_tolerance,
                       const double* accept_tolerance, int n_problems, const mpe_rig_init_options* options,
                       mpe_result* out, uint32_t* match_out, mpe_rig_init_info* info_out) {
  if (!h || n_problems < 0) return fail(h, MPE_ERR_ARG, "bad argument");
  if (!cameras) return fail(h, MPE_ERR_ARG, "cameras is null");
  if (!markers_xyz) return fail(h, MPE_ERR_ARG, "markers_xyz is null");
  if (!det_begin) return fail(h, MPE_ERR_ARG, "det_begin is null");
  if (!vote_tolerance || !accept_tolerance) return fail(h, MPE_ERR_ARG, "a tolerance array is null");
  if (!out) return fail(h, MPE_ERR_ARG, "out is null");
  if (n_cameras < 1 || n_cameras > MPE_RIG_MAX_CAMERAS) return fail(h, MPE_ERR_ARG, "n_cameras outside 1 .. MPE_RIG_MAX_CAMERAS");
  if (n_markers < 1 || n_markers > MPE_MAX_MARKERS) return fail(h, MPE_ERR_ARG, "n_markers outside 1 .. MPE_MAX_MARKERS");
  mpe_rig_init_options opt;
  mpe_rig_init_default_options(&opt);
  if (options) opt = *options;
  if (opt.max_rounds < 1 || opt.max_rounds > 4) return fail(h, MPE_ERR_ARG, "max_rounds outside 1 .. 4");
  if (opt.min_rows < 3) return fail(h, MPE_ERR_ARG, "min_rows must be >= 3");
  if (opt.min_markers < 1) return fail(h, MPE_ERR_ARG, "min_markers must be >= 1");
  if (opt.min_margin < 0) return fail(h, MPE_ERR_ARG, "min_margin must be >= 0");
  for (int c = 0; c < n_cameras; ++c)
    if (!(vote_tolerance[c] > 0) || !(accept_tolerance[c] > 0)) return fail(h, MPE_ERR_ARG, "a tolerance is not > 0");
  if (n_problems == 0) return MPE_OK;
  const size_t n_lists = (size_t)n_problems * (size_t)n_cameras;
  if (det_begin[0] < 0) return fail(h, MPE_ERR_ARG, "det_begin is negative");
  for (size_t i = 0; i < n_lists; ++i)
    if (det_begin[i + 1] < det_begin[i]) return fail(h, MPE_ERR_ARG, "det_begin decreases");
  for (size_t i = 0; i < n_lists; ++i)
    if (det_begin[i + 1] - det_begin[i] > MPE_MAX_DETECTIONS)
      return fail(h, MPE_ERR_UNSUPPORTED, "more than MPE_MAX_DETECTIONS detections in a camera's list");
  // the items of every problem, counted from det_begin alone, and the blocks that vote on them
  const long long perms = n_markers >= 3 ? (long long)n_markers * (n_markers - 1) * (n_markers - 2) : 0;
  std::vector<int> chunk_begin((size_t)n_problems + 1, 0);
  for (int i = 0; i < n_problems; ++i) {
    long long items = 0;
    for (int c = 0; c < n_cameras; ++c) {
      const long long n = det_begin[(size_t)i * n_cameras + c + 1] - det_begin[(size_t)i * n_cameras + c];
      if (n >= 3) items += n * (n - 1) * (n - 2) / 6 * perms;
    }
    if (items > MPE_RIG_INIT_ITEM_CAP) return fail(h, MPE_ERR_UNSUPPORTED, "more than 2^22 items (detection triples x marker permutations) in a problem");
    const long long blocks = (items + MPE_RIG_INIT_BLOCK_ITEMS - 1) / MPE_RIG_INIT_BLOCK_ITEMS;
    if (chunk_begin[(size_t)i] + blocks > 0x7fffffffLL) return fail(h, MPE_ERR_UNSUPPORTED, "more than 2^31 voting blocks in a call");
    chunk_begin[(size_t)i + 1] = chunk_begin[(size_t)i] + (int)blocks;
  }
  const int n_chunks = chunk_begin[(size_t)n_problems];
  const int d0 = det_begin[0], n_det = det_begin[n_lists] - d0;
  if (n_det > 0 && !det_xy) return fail(h, MPE_ERR_ARG, "det_xy is null");
  if (h->pending_track_n || h->submit_seq != h->collect_seq)
    return fail(h, MPE_ERR_ARG, "a submitted batch has not been collected yet");
  ENTER(h);
  // in: [cameras | markers | vote tolerances | accept tolerances | det_begin (rebased to 0) | chunk_begin | detections];
  // back: [records | match words | info records]; on the device only: [keys | winners | runners | winner row sets]
  const size_t cam_bytes = (size_t)n_cameras * sizeof(mpe_rig_camera);
  const size_t mk_off = up256(cam_bytes);
  const size_t tv_off = mk_off + up256((size_t)n_markers * 3 * sizeof(double));
  const size_t ta_off = tv_off + up256((size_t)n_cameras * sizeof(double));
  const size_t beg_off = ta_off + up256((size_t)n_cameras * sizeof(double));
  const size_t chk_off = beg_off + up256((n_lists + 1) * sizeof(int));
  const size_t det_off = chk_off + up256(((size_t)n_problems + 1) * sizeof(int));
  const size_t in_bytes = det_off + up256((size_t)n_det * 2 * sizeof(double));
  const size_t rec_bytes = (size_t)n_problems * sizeof(mpe_result);
  const size_t match_words = n_lists * (size_t)n_markers;
  const size_t m_off = up256(rec_bytes);
  const size_t i_off = m_off + up256(match_words * sizeof(uint32_t));
  const size_t back_bytes = i_off + (size_t)n_problems * sizeof(mpe_rig_init_info);
  const size_t back_off = up256(in_bytes);
  const size_t win_off = up256((size_t)n_chunks * MPE_RIG_INIT_KEY_BYTES);
  const size_t run_off = win_off + up256((size_t)n_problems * MPE_RIG_INIT_KEY_BYTES);
  const size_t rows_off = run_off + up256((size_t)n_chunks * sizeof(int));
  const size_t work_bytes = rows_off + (size_t)n_problems * MPE_RIG_MAX_CAMERAS * MPE_MAX_MARKERS;
  { const int rc = grow_mailbox(h, back_off + back_bytes); if (rc != MPE_OK) return rc; }
  uint8_t* mb = static_cast<uint8_t*>(h->mailbox);
  std::memcpy(mb, cameras, cam_bytes);
  std::memcpy(mb + mk_off, markers_xyz, (size_t)n_markers * 3 * sizeof(double));
  std::memcpy(mb + tv_off, vote_tolerance, (size_t)n_cameras * sizeof(double));
  std::memcpy(mb + ta_off, accept_tolerance, (size_t)n_cameras * sizeof(double));
  int* hb = reinterpret_cast<int*>(mb + beg_off);
  for (size_t i = 0; i <= n_lists; ++i) hb[i] = det_begin[i] - d0;
  std::memcpy(mb + chk_off, chunk_begin.data(), chunk_begin.size() * sizeof(int));
  if (n_det > 0) std::memcpy(mb + det_off, det_xy + (size_t)2 * d0, (size_t)n_det * 2 * sizeof(double));
  HIP_TRY(h, h->frames.reserve(in_bytes));
  HIP_TRY(h, h->results.reserve(back_bytes));
  HIP_TRY(h, h->scratch.reserve(work_bytes));
  uint8_t* d_in = static_cast<uint8_t*>(h->frames.p);
  uint8_t* d_back = static_cast<uint8_t*>(h->results.p);
  uint8_t* d_work = static_cast<uint8_t*>(h->scratch.p);
  HIP_TRY(h, hipMemcpyAsync(d_in, mb, in_bytes, hipMemcpyHostToDevice, h->stream));
  RigInitDev d;
  d.cams = reinterpret_cast<const mpe_rig_camera*>(d_in);
  d.markers = reinterpret_cast<const double*>(d_in + mk_off);
  d.det_xy = reinterpret_cast<const double*>(d_in + det_off);
  d.tol_vote = reinterpret_cast<const double*>(d_in + tv_off);
  d.tol_accept = reinterpret_cast<const double*>(d_in + ta_off);
  d.det_begin = reinterpret_cast<const int*>(d_in + beg_off);
  d.chunk_begin = reinterpret_cast<const int*>(d_in + chk_off);
  d.n_cam = n_cameras, d.n_markers = n_markers, d.n_problems = n_problems, d.n_chunks = n_chunks;
  d.max_rounds = opt.max_rounds, d.min_rows = opt.min_rows, d.min_markers = opt.min_markers, d.min_margin = opt.min_margin;
  d.keys = reinterpret_cast<RigInitKey*>(d_work);
  d.winner = reinterpret_cast<RigInitKey*>(d_work + win_off);
  d.runners = reinterpret_cast<int*>(d_work + run_off);
  d.win_rows = d_work + rows_off;
  d.out = reinterpret_cast<mpe_result*>(d_back);
  d.match = reinterpret_cast<uint32_t*>(d_back + m_off);
  d.info = reinterpret_cast<mpe_rig_init_info*>(d_back + i_off);
  RigLaunchTimer timer(h);
  HIP_TRY(h, timer.begin());
  HIP_TRY(h, launch_k_rig_init(d, h->stream));
  HIP_TRY(h, timer.end());
  ++h->rig_init_submits;
  HIP_TRY(h, hipMemcpyAsync(mb + back_off, d_back, back_bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  timer.read();
  std::memcpy(out, mb + back_off, rec_bytes);
  if (match_out) std::memcpy(match_out, mb + back_off + m_off, match_words * sizeof(uint32_t));
  if (info_out) std::memcpy(info_out, mb + back_off + i_off, (size_t)n_problems * sizeof(mpe_rig_init_info));
  return MPE_OK;
}

void mpe_rig_init_bodies_default_options(mpe_rig_init_options* o, int n_cameras, int n_markers) {
  if (!o) return;
  mpe_rig_init_default_options(o);
  o->min_margin = 0;  // (an identical second body always contradicts the winner with equal rows)
  if (n_cameras <= 1) o->min_rows = o->min_markers = n_markers;
}

int mpe_rig_init_bodies_batch(mpe_handle* h, const mpe_rig_camera* cameras, int n_cameras, const mpe_rig_body* bodies,
                              int n_bodies, const int* det_begin, const double* det_xy, const uint8_t* claimed_in,
                              const uint8_t* find, const double* vote_tolerance, const double* accept_tolerance,
                              int n_problems, mpe_result* out, uint32_t* match_out, mpe_rig_init_info* info_out,
                              int8_t* owner_out) {
  // (the handle is looked at behind everything that can be refused without it)
  if (n_problems < 0) return fail(h, MPE_ERR_ARG, "bad argument");
  if (!cameras) return fail(h, MPE_ERR_ARG, "cameras is null");
  if (!bodies) return fail(h, MPE_ERR_ARG, "bodies is null");
  if (!det_begin) return fail(h, MPE_ERR_ARG, "det_begin is null");
  if (!vote_tolerance || !accept_tolerance) return fail(h, MPE_ERR_ARG, "a tolerance array is null");
  if (!out) return fail(h, MPE_ERR_ARG, "out is null");
  if (n_cameras < 1 || n_cameras > MPE_RIG_MAX_CAMERAS) return fail(h, MPE_ERR_ARG, "n_cameras outside 1 .. MPE_RIG_MAX_CAMERAS");
  if (n_bodies < 1 || n_bodies > MPE_MAX_BODIES) return fail(h, MPE_ERR_ARG, "n_bodies outside 1 .. MPE_MAX_BODIES");
  std::vector<mpe_rig_init_options> opts((size_t)n_bodies);
  for (int b = 0; b < n_bodies; ++b) {
    if (!bodies[b].markers_xyz) return fail(h, MPE_ERR_ARG, "markers_xyz of a body is null");
    if (bodies[b].n_markers < 1 || bodies[b].n_markers > MPE_MAX_MARKERS) return fail(h, MPE_ERR_ARG, "n_markers of a body outside 1 .. MPE_MAX_MARKERS");
    mpe_rig_init_options& opt = opts[(size_t)b];
    mpe_rig_init_bodies_default_options(&opt, n_cameras, bodies[b].n_markers);
    if (bodies[b].options) opt = *bodies[b].options;
    if (opt.max_rounds < 1 || opt.max_rounds > 4) return fail(h, MPE_ERR_ARG, "max_rounds outside 1 .. 4");
    if (opt.min_rows < 3) return fail(h, MPE_ERR_ARG, "min_rows must be >= 3");
    if (opt.min_markers < 1) return fail(h, MPE_ERR_ARG, "min_markers must be >= 1");
    if (opt.min_margin < 0) return fail(h, MPE_ERR_ARG, "min_margin must be >= 0");
  }
  for (int c = 0; c < n_cameras; ++c)
    if (!(vote_tolerance[c] > 0) || !(accept_tolerance[c] > 0)) return fail(h, MPE_ERR_ARG, "a tolerance is not > 0");
  if (n_problems == 0) return MPE_OK;
  const size_t n_lists = (size_t)n_problems * (size_t)n_cameras;
  if (det_begin[0] < 0) return fail(h, MPE_ERR_ARG, "det_begin is negative");
  for (size_t i = 0; i < n_lists; ++i)
    if (det_begin[i + 1] < det_begin[i]) return fail(h, MPE_ERR_ARG, "det_begin decreases");
  for (size_t i = 0; i < n_lists; ++i)
    if (det_begin[i + 1] - det_begin[i] > MPE_MAX_DETECTIONS)
      return fail(h, MPE_ERR_UNSUPPORTED, "more than MPE_MAX_DETECTIONS detections in a camera's list");
  const int d0 = det_begin[0], n_det = det_begin[n_lists] - d0;
  if (n_det > 0 && !det_xy) return fail(h, MPE_ERR_ARG, "det_xy is null");
  // what claimed_in leaves of every list
  std::vector<int> n_left(n_lists);
  for (size_t l = 0; l < n_lists; ++l) {
    int n = 0;
    for (int k = det_begin[l]; k < det_begin[l + 1]; ++k) n += (!claimed_in || claimed_in[k] == 0) ? 1 : 0;
    n_left[l] = n;
  }
  // The voting blocks of every round, counted ONCE per body from the lists claimed_in leaves: an upper bound for the
  // round itself, whose lists the earlier rounds have only shortened.  The kernels allow that as they are:
  // k_rig_init_vote takes its item count from the lists it staged (S.off[n_cam]), a block beyond that count writes
  // rig_init_no_key() / runner 0, and k_rig_init_winner / _finish reduce over whatever blocks there are — the keys are
  // totally ordered, so the surplus blocks do not show.  A body that is not asked for in a problem gets no block there.
  std::vector<int> chunk_begin((size_t)n_bodies * ((size_t)n_problems + 1), 0);
  int max_chunks = 0;
  for (int b = 0; b < n_bodies; ++b) {
    const long long nm = bodies[b].n_markers;
    const long long perms = nm >= 3 ? nm * (nm - 1) * (nm - 2) : 0;
    int* cb = chunk_begin.data() + (size_t)b * ((size_t)n_problems + 1);
    for (int i = 0; i < n_problems; ++i) {
      long long items = 0;
      if (!find || find[(size_t)i * n_bodies + b] != 0)
        for (int c = 0; c < n_cameras; ++c) {
          const long long n = n_left[(size_t)i * n_cameras + c];
          if (n >= 3) items += n * (n - 1) * (n - 2) / 6 * perms;
        }
      if (items > MPE_RIG_INIT_ITEM_CAP) return fail(h, MPE_ERR_UNSUPPORTED, "more than 2^22 items (detection triples x marker permutations) for a body in a problem");
      const long long blocks = (items + MPE_RIG_INIT_BLOCK_ITEMS - 1) / MPE_RIG_INIT_BLOCK_ITEMS;
      if (cb[i] + blocks > 0x7fffffffLL) return fail(h, MPE_ERR_UNSUPPORTED, "more than 2^31 voting blocks in a round");
      cb[i + 1] = cb[i] + (int)blocks;
    }
    max_chunks = cb[n_problems] > max_chunks ? cb[n_problems] : max_chunks;
  }
  if (!h) return fail(h, MPE_ERR_ARG, "bad argument");
  if (h->pending_track_n || h->submit_seq != h->collect_seq)
    return fail(h, MPE_ERR_ARG, "a submitted batch has not been collected yet");
  ENTER(h);
  // in: [cameras | vote tolerances | accept tolerances | det_begin (rebased to 0) | detections | owner bytes at entry |
  // find | per body: markers, chunk_begin]; back: [records | match words | info records | owner bytes]; on the device
  // only: the rounds' [keys | winners | runners | winner row sets], the round's lists [counts | det_begin | index map |
  // detections] and the round's answer [records | match words | info records]
  const size_t n_rec = (size_t)n_problems * (size_t)n_bodies;
  const size_t cam_bytes = (size_t)n_cameras * sizeof(mpe_rig_camera);
  const size_t tv_off = up256(cam_bytes);
  const size_t ta_off = tv_off + up256((size_t)n_cameras * sizeof(double));
  const size_t beg_off = ta_off + up256((size_t)n_cameras * sizeof(double));
  const size_t det_off = beg_off + up256((n_lists + 1) * sizeof(int));
  const size_t own_off = det_off + up256((size_t)n_det * 2 * sizeof(double));
  const size_t find_off = own_off + up256((size_t)n_det);
  const size_t body_off = find_off + up256(n_rec);
  const size_t mk_bytes = up256((size_t)MPE_MAX_MARKERS * 3 * sizeof(double));
  const size_t body_bytes = mk_bytes + up256(((size_t)n_problems + 1) * sizeof(int));
  const size_t in_bytes = body_off + (size_t)n_bodies * body_bytes;
  const size_t rec_bytes = n_rec * sizeof(mpe_result);
  const size_t match_words = n_rec * (size_t)n_cameras * MPE_MAX_MARKERS;
  const size_t m_off = up256(rec_bytes);
  const size_t i_off = m_off + up256(match_words * sizeof(uint32_t));
  const size_t o_off = i_off + up256(n_rec * sizeof(mpe_rig_init_info));
  const size_t back_bytes = o_off + up256((size_t)n_det);
  const size_t back_off = up256(in_bytes);
  const size_t win_off = up256((size_t)max_chunks * MPE_RIG_INIT_KEY_BYTES);
  const size_t run_off = win_off + up256((size_t)n_problems * MPE_RIG_INIT_KEY_BYTES);
  const size_t rows_off = run_off + up256((size_t)max_chunks * sizeof(int));
  const size_t cnt_off = rows_off + up256((size_t)n_problems * MPE_RIG_MAX_CAMERAS * MPE_MAX_MARKERS);
  const size_t rbeg_off = cnt_off + up256(n_lists * sizeof(int));
  const size_t map_off = rbeg_off + up256((n_lists + 1) * sizeof(int));
  const size_t rxy_off = map_off + up256((size_t)n_det * sizeof(int));
  const size_t rrec_off = rxy_off + up256((size_t)n_det * 2 * sizeof(double));
  const size_t rm_off = rrec_off + up256((size_t)n_problems * sizeof(mpe_result));
  const size_t ri_off = rm_off + up256(n_lists * MPE_MAX_MARKERS * sizeof(uint32_t));
  const size_t work_bytes = ri_off + up256((size_t)n_problems * sizeof(mpe_rig_init_info));
  { const int rc = grow_mailbox(h, back_off + back_bytes); if (rc != MPE_OK) return rc; }
  uint8_t* mb = static_cast<uint8_t*>(h->mailbox);
  std::memcpy(mb, cameras, cam_bytes);
  std::memcpy(mb + tv_off, vote_tolerance, (size_t)n_cameras * sizeof(double));
  std::memcpy(mb + ta_off, accept_tolerance, (size_t)n_cameras * sizeof(double));
  int* hb = reinterpret_cast<int*>(mb + beg_off);
  for (size_t i = 0; i <= n_lists; ++i) hb[i] = det_begin[i] - d0;
  if (n_det > 0) std::memcpy(mb + det_off, det_xy + (size_t)2 * d0, (size_t)n_det * 2 * sizeof(double));
  for (int k = 0; k < n_det; ++k) reinterpret_cast<int8_t*>(mb + own_off)[k] = (claimed_in && claimed_in[d0 + k] != 0) ? -2 : -1;
  for (size_t k = 0; k < n_rec; ++k) mb[find_off + k] = (!find || find[k] != 0) ? 1 : 0;
  for (int b = 0; b < n_bodies; ++b) {
    uint8_t* p = mb + body_off + (size_t)b * body_bytes;
    std::memcpy(p, bodies[b].markers_xyz, (size_t)bodies[b].n_markers * 3 * sizeof(double));
    std::memcpy(p + mk_bytes, chunk_begin.data() + (size_t)b * ((size_t)n_problems + 1), ((size_t)n_problems + 1) * sizeof(int));
  }
  HIP_TRY(h, h->frames.reserve(in_bytes));
  HIP_TRY(h, h->results.reserve(back_bytes));
  HIP_TRY(h, h->scratch.reserve(work_bytes));
  uint8_t* d_in = static_cast<uint8_t*>(h->frames.p);
  uint8_t* d_back = static_cast<uint8_t*>(h->results.p);
  uint8_t* d_work = static_cast<uint8_t*>(h->scratch.p);
  HIP_TRY(h, hipMemcpyAsync(d_in, mb, in_bytes, hipMemcpyHostToDevice, h->stream));
  RigPeelDev p;
  p.det_begin = reinterpret_cast<const int*>(d_in + beg_off);
  p.det_xy = reinterpret_cast<const double*>(d_in + det_off);
  p.owner_in = reinterpret_cast<const int8_t*>(d_in + own_off);
  p.find = d_in + find_off;
  p.n_cam = n_cameras, p.n_problems = n_problems, p.n_bodies = n_bodies;
  p.counts = reinterpret_cast<int*>(d_work + cnt_off);
  p.r_begin = reinterpret_cast<int*>(d_work + rbeg_off);
  p.map = reinterpret_cast<int*>(d_work + map_off);
  p.r_xy = reinterpret_cast<double*>(d_work + rxy_off);
  mpe_result* r_out = reinterpret_cast<mpe_result*>(d_work + rrec_off);
  uint32_t* r_match = reinterpret_cast<uint32_t*>(d_work + rm_off);
  mpe_rig_init_info* r_info = reinterpret_cast<mpe_rig_init_info*>(d_work + ri_off);
  p.r_out = r_out, p.r_match = r_match, p.r_info = r_info;
  p.out = reinterpret_cast<mpe_result*>(d_back);
  p.match = reinterpret_cast<uint32_t*>(d_back + m_off);
  p.info = reinterpret_cast<mpe_rig_init_info*>(d_back + i_off);
  p.owner = reinterpret_cast<int8_t*>(d_back + o_off);
  RigLaunchTimer timer(h);
  HIP_TRY(h, timer.begin());
  for (int b = 0; b <= n_bodies; ++b) {
    // the claims and the answer of round b - 1, then (b < n_bodies) the lists of round b
    HIP_TRY(h, launch_k_rig_peel(p, b, b > 0 ? bodies[b - 1].n_markers : 0, h->stream));
    if (b == n_bodies) break;
    const uint8_t* body = d_in + body_off + (size_t)b * body_bytes;
    RigInitDev d;
    d.cams = reinterpret_cast<const mpe_rig_camera*>(d_in);
    d.markers = reinterpret_cast<const double*>(body);
    d.det_xy = p.r_xy;
    d.tol_vote = reinterpret_cast<const double*>(d_in + tv_off);
    d.tol_accept = reinterpret_cast<const double*>(d_in + ta_off);
    d.det_begin = p.r_begin;
    d.chunk_begin = reinterpret_cast<const int*>(body + mk_bytes);
    d.n_cam = n_cameras, d.n_markers = bodies[b].n_markers, d.n_problems = n_problems;
    d.n_chunks = chunk_begin[(size_t)b * ((size_t)n_problems + 1) + (size_t)n_problems];
    const mpe_rig_init_options& opt = opts[(size_t)b];
    d.max_rounds = opt.max_rounds, d.min_rows = opt.min_rows, d.min_markers = opt.min_markers, d.min_margin = opt.min_margin;
    d.keys = reinterpret_cast<RigInitKey*>(d_work);
    d.winner = reinterpret_cast<RigInitKey*>(d_work + win_off);
    d.runners = reinterpret_cast<int*>(d_work + run_off);
    d.win_rows = d_work + rows_off;
    d.out = r_out, d.match = r_match, d.info = r_info;
    HIP_TRY(h, launch_k_rig_init(d, h->stream));
  }
  HIP_TRY(h, timer.end());
  ++h->rig_init_bodies_submits;
  HIP_TRY(h, hipMemcpyAsync(mb + back_off, d_back, back_bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  timer.read();
  std::memcpy(out, mb + back_off, rec_bytes);
  if (match_out) std::memcpy(match_out, mb + back_off + m_off, match_words * sizeof(uint32_t));
  if (info_out) std::memcpy(info_out, mb + back_off + i_off, n_rec * sizeof(mpe_rig_init_info));
  if (owner_out && n_det > 0) std::memcpy(owner_out + d0, mb + back_off + o_off, (size_t)n_det);
  return MPE_OK;
}

void mpe_rig_calibration_default_options(mpe_rig_calibration_options* o) {
  if (!o) return;
  o->reference_camera = 0;
  o->max_iterations = 50;
  o->step_tolerance = 1e-10;
}

int mpe_rig_calibrate(mpe_handle* h, const mpe_rig_camera* cameras, int n_cameras, const int* view_begin,
                      const int* row_camera, const double* row_marker_xyz, const double* row_uv, int n_views,
                      const double* T_view_init, const mpe_rig_calibration_options* options, double* T_cam_rig_out,
                      double* T_view_out, double* cov_out, int* view_used, mpe_rig_calibration_report* report) {
  if (!h || n_views < 0) return fail(h, MPE_ERR_ARG, "bad argument");
  if (!cameras) return fail(h, MPE_ERR_ARG, "cameras is null");
  if (!view_begin) return fail(h, MPE_ERR_ARG, "view_begin is null");
  if (!T_cam_rig_out) return fail(h, MPE_ERR_ARG, "T_cam_rig_out is null");
  if (!report) return fail(h, MPE_ERR_ARG, "report is null");
  if (n_views > 0 && !T_view_init) return fail(h, MPE_ERR_ARG, "T_view_init is null");
  if (n_cameras < 1 || n_cameras > MPE_RIG_MAX_CAMERAS) return fail(h, MPE_ERR_ARG, "n_cameras outside 1 .. MPE_RIG_MAX_CAMERAS");
  mpe_rig_calibration_options opt;
  mpe_rig_calibration_default_options(&opt);
  if (options) opt = *options;
  if (opt.reference_camera < 0 || opt.reference_camera >= n_cameras) return fail(h, MPE_ERR_ARG, "reference_camera outside the rig");
  if (opt.max_iterations < 1) return fail(h, MPE_ERR_ARG, "max_iterations must be >= 1");
  if (!(opt.step_tolerance > 0)) return fail(h, MPE_ERR_ARG, "step_tolerance must be positive");
  if (view_begin[0] < 0) return fail(h, MPE_ERR_ARG, "view_begin is negative");
  for (int f = 0; f < n_views; ++f) {
    if (view_begin[f + 1] < view_begin[f]) return fail(h, MPE_ERR_ARG, "view_begin decreases");
    if (view_begin[f + 1] - view_begin[f] > MPE_RIG_MAX_CAMERAS * MPE_MAX_MARKERS)
      return fail(h, MPE_ERR_UNSUPPORTED, "more than MPE_RIG_MAX_CAMERAS * MPE_MAX_MARKERS rows in a view");
  }
  const int r0 = view_begin[0], r1 = view_begin[n_views];
  if (r1 > r0 && (!row_camera || !row_marker_xyz || !row_uv)) return fail(h, MPE_ERR_ARG, "a row array is null");
  for (int j = r0; j < r1; ++j)
    if (row_camera[j] < 0 || row_camera[j] >= n_cameras) return fail(h, MPE_ERR_ARG, "camera index outside the rig");
  if (h->pending_track_n || h->submit_seq != h->collect_seq)
    return fail(h, MPE_ERR_ARG, "a submitted batch has not been collected yet");

  RigBaPlan P;
  rig_ba_plan(n_cameras, opt.reference_camera, view_begin, row_camera, row_marker_xyz, row_uv, n_views, MPE_RIG_BA_HEAD,
              MPE_RIG_BA_SLOT, P);
  rig_ba_give_back(P, cameras, n_views, T_view_init, T_cam_rig_out, T_view_out, cov_out, view_used, report);
  if (P.views_used == 0 || P.n_free == 0) return 0;

  ENTER(h);
  const int nv = P.views_used, nr = P.rows_used, nf = P.n_free;
  // one block of device memory: [cameras | free index | view_begin | masks | record offsets | row cameras | marker xyz |
  // pixels | view poses] from the host, then what the steps keep among themselves
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += up256(bytes);
    return o;
  };
  const size_t o_cam = take((size_t)n_cameras * sizeof(mpe_rig_camera)), o_free = take(16 * sizeof(int)),
               o_beg = take((size_t)(nv + 1) * sizeof(int)), o_mask = take((size_t)nv * sizeof(unsigned)),
               o_cum = take((size_t)(nv + 1) * sizeof(long long)), o_rc = take((size_t)nr * sizeof(int)),
               o_xyz = take((size_t)nr * 3 * sizeof(double)), o_uv = take((size_t)nr * 2 * sizeof(double)),
               o_T = take((size_t)nv * 16 * sizeof(double));
  const size_t in_bytes = off;
  const size_t o_cov = take((size_t)nf * 36 * sizeof(double)), o_out = take(2 * sizeof(double));
  const size_t back_end = off;  // [o_cam, in_bytes) and [o_cov, back_end) come back
  const size_t o_sse = take((size_t)nv * sizeof(double)), o_step = take((size_t)nv * sizeof(double)),
               o_S = take((size_t)(nf * (nf + 1) / 2) * 72 * sizeof(double)), o_r = take((size_t)nf * 12 * sizeof(double)),
               o_L = take((size_t)MPE_RIG_BA_TRI * sizeof(double)), o_eta = take((size_t)MPE_RIG_BA_MAX_N * sizeof(double));
  const size_t dev_bytes = off;
  { const int rc = grow_mailbox(h, back_end); if (rc != MPE_OK) return rc; }
  uint8_t* mb = static_cast<uint8_t*>(h->mailbox);
  std::memset(mb, 0, in_bytes);
  std::memcpy(mb + o_cam, cameras, (size_t)n_cameras * sizeof(mpe_rig_camera));
  std::memcpy(mb + o_free, P.cam_free, 16 * sizeof(int));
  std::memcpy(mb + o_beg, P.view_begin.data(), (size_t)(nv + 1) * sizeof(int));
  std::memcpy(mb + o_mask, P.view_mask.data(), (size_t)nv * sizeof(unsigned));
  std::memcpy(mb + o_cum, P.view_cum.data(), (size_t)(nv + 1) * sizeof(long long));
  std::memcpy(mb + o_rc, P.row_cam.data(), (size_t)nr * sizeof(int));
  std::memcpy(mb + o_xyz, P.row_xyz.data(), (size_t)nr * 3 * sizeof(double));
  std::memcpy(mb + o_uv, P.row_uv.data(), (size_t)nr * 2 * sizeof(double));
  for (int v = 0; v < nv; ++v)
    std::memcpy(mb + o_T + (size_t)v * 16 * sizeof(double), T_view_init + 16 * (size_t)P.view_of[(size_t)v], 16 * sizeof(double));
  // the records of one chunk of views
  const long long cap_doubles = (long long)(h->rig_ba_record_kb > 0 ? h->rig_ba_record_kb : 65536) * 1024 / 8;
  const std::vector<std::pair<int, int>> chunks = rig_ba_chunks(P, cap_doubles);
  long long rec_doubles = 0;
  for (const auto& c : chunks)
    rec_doubles = std::max(rec_doubles, P.view_cum[(size_t)(c.first + c.second)] - P.view_cum[(size_t)c.first]);
  HIP_TRY(h, h->frames.reserve(dev_bytes));
  HIP_TRY(h, h->scratch.reserve((size_t)rec_doubles * sizeof(double)));
  uint8_t* dv = static_cast<uint8_t*>(h->frames.p);
  HIP_TRY(h, hipMemcpyAsync(dv, mb, in_bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemsetAsync(dv + o_cov, 0, (size_t)nf * 36 * sizeof(double), h->stream));
  BaLaunches<RigBaDev, launch_k_rig_ba> B;
  B.h = h;
  B.ms = h->rig_ba_ms, B.launches = &h->rig_ba_launches;
  B.host_out = reinterpret_cast<double*>(mb + o_out);
  RigBaDev& d = B.d;
  d.cams = reinterpret_cast<mpe_rig_camera*>(dv + o_cam);
  d.cam_free = reinterpret_cast<const int*>(dv + o_free);
  d.n_cam = n_cameras, d.n_free = nf, d.n_views = nv;
  d.view_begin = reinterpret_cast<const int*>(dv + o_beg);
  d.view_mask = reinterpret_cast<const unsigned*>(dv + o_mask);
  d.view_cum = reinterpret_cast<const long long*>(dv + o_cum);
  d.row_cam = reinterpret_cast<const int*>(dv + o_rc);
  d.row_xyz = reinterpret_cast<const double*>(dv + o_xyz);
  d.row_uv = reinterpret_cast<const double*>(dv + o_uv);
  d.T_view = reinterpret_cast<double*>(dv + o_T);
  d.rec = static_cast<double*>(h->scratch.p);
  d.sse = reinterpret_cast<double*>(dv + o_sse);
  d.step = reinterpret_cast<double*>(dv + o_step);
  d.Sacc = reinterpret_cast<double*>(dv + o_S);
  d.racc = reinterpret_cast<double*>(dv + o_r);
  d.Lf = reinterpret_cast<double*>(dv + o_L);
  d.eta = reinterpret_cast<double*>(dv + o_eta);
  d.cov = reinterpret_cast<double*>(dv + o_cov);
  d.out = reinterpret_cast<double*>(dv + o_out);
  RigBaOutcome o;
  if (rig_ba_iterate(B, chunks, opt.max_iterations, opt.step_tolerance, o)) return fail(h, MPE_ERR_HIP, "mpe_rig_calibrate", B.err);
  HIP_TRY(h, hipMemcpyAsync(mb + o_cam, dv + o_cam, (size_t)n_cameras * sizeof(mpe_rig_camera), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(mb + o_T, dv + o_T, (size_t)nv * 16 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(mb + o_cov, dv + o_cov, (size_t)nf * 36 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  B.read_out();
  const mpe_rig_camera* cam_back = reinterpret_cast<const mpe_rig_camera*>(mb + o_cam);
  const double* T_back = reinterpret_cast<const double*>(mb + o_T);
  const double* cov_back = reinterpret_cast<const double*>(mb + o_cov);
  return rig_ba_hand_out(P, o, cam_back, T_back, cov_back, T_cam_rig_out, T_view_out, cov_out, report);
}

void mpe_body_calibration_default_options(mpe_body_calibration_options* o) {
  if (!o) return;
  o->scale = -1;
  o->max_iterations = 50;
  o->step_tolerance = 1e-10;
}

int mpe_body_calibrate(mpe_handle* h, const mpe_rig_camera* cameras, int n_cameras, const double* markers_xyz,
                       int n_markers, const int* view_begin, const int* row_camera, const int* row_marker,
                       const double* row_uv, int n_views, const double* T_view_init,
                       const mpe_body_calibration_options* options, double* markers_out, double* T_view_out,
                       double* cov_out, int* view_used, mpe_body_calibration_report* report) {
  if (!h || n_views < 0) return fail(h, MPE_ERR_ARG, "bad argument");
  if (!cameras) return fail(h, MPE_ERR_ARG, "cameras is null");
  if (!markers_xyz) return fail(h, MPE_ERR_ARG, "markers_xyz is null");
  if (!view_begin) return fail(h, MPE_ERR_ARG, "view_begin is null");
  if (!markers_out) return fail(h, MPE_ERR_ARG, "markers_out is null");
  if (!report) return fail(h, MPE_ERR_ARG, "report is null");
  if (n_views > 0 && !T_view_init) return fail(h, MPE_ERR_ARG, "T_view_init is null");
  if (n_cameras < 1 || n_cameras > MPE_RIG_MAX_CAMERAS) return fail(h, MPE_ERR_ARG, "n_cameras outside 1 .. MPE_RIG_MAX_CAMERAS");
  if (n_markers < 1 || n_markers > MPE_MAX_MARKERS) return fail(h, MPE_ERR_ARG, "n_markers outside 1 .. MPE_MAX_MARKERS");
  mpe_body_calibration_options opt;
  mpe_body_calibration_default_options(&opt);
  if (options) opt = *options;
  if (opt.scale < -1 || opt.scale > 1) return fail(h, MPE_ERR_ARG, "scale outside -1 .. 1");
  if (opt.max_iterations < 1) return fail(h, MPE_ERR_ARG, "max_iterations must be >= 1");
  if (!(opt.step_tolerance > 0)) return fail(h, MPE_ERR_ARG, "step_tolerance must be positive");
  if (view_begin[0] < 0) return fail(h, MPE_ERR_ARG, "view_begin is negative");
  for (int f = 0; f < n_views; ++f)
    if (view_begin[f + 1] < view_begin[f]) return fail(h, MPE_ERR_ARG, "view_begin decreases");
  const int r0 = view_begin[0], r1 = view_begin[n_views];
  if (r1 > r0 && (!row_camera || !row_marker || !row_uv)) return fail(h, MPE_ERR_ARG, "a row array is null");
  for (int j = r0; j < r1; ++j) {
    if (row_camera[j] < 0 || row_camera[j] >= n_cameras) return fail(h, MPE_ERR_ARG, "camera index outside the rig");
    if (row_marker[j] < 0 || row_marker[j] >= n_markers) return fail(h, MPE_ERR_ARG, "marker index outside the marker set");
  }
  if (h->pending_track_n || h->submit_seq != h->collect_seq)
    return fail(h, MPE_ERR_ARG, "a submitted batch has not been collected yet");
  for (int f = 0; f < n_views; ++f)
    if (view_begin[f + 1] - view_begin[f] > MPE_RIG_MAX_CAMERAS * MPE_MAX_MARKERS)
      return fail(h, MPE_ERR_UNSUPPORTED, "more than MPE_RIG_MAX_CAMERAS * MPE_MAX_MARKERS rows in a view");

  BodyBaPlan P;
  body_ba_plan(n_markers, view_begin, row_camera, row_marker, row_uv, n_views, MPE_BODY_BA_HEAD, MPE_BODY_BA_SLOT, P);
  const int held = body_ba_scale_held(P, opt.scale);
  body_ba_give_back(P, held, markers_xyz, n_views, T_view_init, markers_out, T_view_out, cov_out, view_used, report);
  if (P.views_used == 0 || P.n_free < 3) return 0;

  ENTER(h);
  const int nv = P.views_used, nr = P.rows_used, nf = P.n_free;
  // one block of device memory: [cameras | free markers | view_begin | masks | record offsets | row cameras | row markers
  // | pixels | marker positions | view poses] from the host, then what the steps keep among themselves
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += up256(bytes);
    return o;
  };
  const size_t o_cam = take((size_t)n_cameras * sizeof(mpe_rig_camera)), o_free = take(16 * sizeof(int)),
               o_beg = take((size_t)(nv + 1) * sizeof(int)), o_mask = take((size_t)nv * sizeof(unsigned)),
               o_cum = take((size_t)(nv + 1) * sizeof(long long)), o_rc = take((size_t)nr * sizeof(int)),
               o_rf = take((size_t)nr * sizeof(int)), o_uv = take((size_t)nr * 2 * sizeof(double)),
               o_mk = take((size_t)n_markers * 3 * sizeof(double)), o_T = take((size_t)nv * 16 * sizeof(double));
  const size_t in_bytes = off;
  const size_t o_cov = take((size_t)nf * 9 * sizeof(double)), o_out = take(2 * sizeof(double));
  const size_t back_end = off;  // [o_mk, in_bytes) and [o_cov, back_end) come back
  const size_t o_sse = take((size_t)nv * sizeof(double)), o_step = take((size_t)nv * sizeof(double)),
               o_S = take((size_t)(nf * (nf + 1) / 2) * 18 * sizeof(double)), o_r = take((size_t)nf * 6 * sizeof(double)),
               o_L = take((size_t)MPE_BODY_BA_TRI * sizeof(double)), o_delta = take((size_t)MPE_BODY_BA_MAX_N * sizeof(double)),
               o_gauge = take((size_t)MPE_BODY_BA_GAUGE * sizeof(double));
  const size_t dev_bytes = off;
  { const int rc = grow_mailbox(h, back_end); if (rc != MPE_OK) return rc; }
  uint8_t* mb = static_cast<uint8_t*>(h->mailbox);
  std::memset(mb, 0, in_bytes);
  std::memcpy(mb + o_cam, cameras, (size_t)n_cameras * sizeof(mpe_rig_camera));
  std::memcpy(mb + o_free, P.free_marker, 16 * sizeof(int));
  std::memcpy(mb + o_beg, P.view_begin.data(), (size_t)(nv + 1) * sizeof(int));
  std::memcpy(mb + o_mask, P.view_mask.data(), (size_t)nv * sizeof(unsigned));
  std::memcpy(mb + o_cum, P.view_cum.data(), (size_t)(nv + 1) * sizeof(long long));
  std::memcpy(mb + o_rc, P.row_cam.data(), (size_t)nr * sizeof(int));
  std::memcpy(mb + o_rf, P.row_free.data(), (size_t)nr * sizeof(int));
  std::memcpy(mb + o_uv, P.row_uv.data(), (size_t)nr * 2 * sizeof(double));
  std::memcpy(mb + o_mk, markers_xyz, (size_t)n_markers * 3 * sizeof(double));
  for (int v = 0; v < nv; ++v)
    std::memcpy(mb + o_T + (size_t)v * 16 * sizeof(double), T_view_init + 16 * (size_t)P.view_of[(size_t)v], 16 * sizeof(double));
  // the records of one chunk of views
  const long long cap_doubles = (long long)(h->rig_ba_record_kb > 0 ? h->rig_ba_record_kb : 65536) * 1024 / 8;
  const std::vector<std::pair<int, int>> chunks = rig_ba_chunks(P, cap_doubles);
  long long rec_doubles = 0;
  for (const auto& c : chunks)
    rec_doubles = std::max(rec_doubles, P.view_cum[(size_t)(c.first + c.second)] - P.view_cum[(size_t)c.first]);
  HIP_TRY(h, h->frames.reserve(dev_bytes));
  HIP_TRY(h, h->scratch.reserve((size_t)rec_doubles * sizeof(double)));
  uint8_t* dv = static_cast<uint8_t*>(h->frames.p);
  HIP_TRY(h, hipMemcpyAsync(dv, mb, in_bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemsetAsync(dv + o_cov, 0, (size_t)nf * 9 * sizeof(double), h->stream));
  BaLaunches<BodyBaDev, launch_k_body_ba> B;
  B.h = h;
  B.ms = h->body_ba_ms, B.launches = &h->body_ba_launches;
  B.host_out = reinterpret_cast<double*>(mb + o_out);
  BodyBaDev& d = B.d;
  d.cams = reinterpret_cast<const mpe_rig_camera*>(dv + o_cam);
  d.free_marker = reinterpret_cast<const int*>(dv + o_free);
  d.n_cam = n_cameras, d.n_free = nf, d.n_views = nv;
  d.scale_held = held;
  d.view_begin = reinterpret_cast<const int*>(dv + o_beg);
  d.view_mask = reinterpret_cast<const unsigned*>(dv + o_mask);
  d.view_cum = reinterpret_cast<const long long*>(dv + o_cum);
  d.row_cam = reinterpret_cast<const int*>(dv + o_rc);
  d.row_free = reinterpret_cast<const int*>(dv + o_rf);
  d.row_uv = reinterpret_cast<const double*>(dv + o_uv);
  d.markers = reinterpret_cast<double*>(dv + o_mk);
  d.T_view = reinterpret_cast<double*>(dv + o_T);
  d.rec = static_cast<double*>(h->scratch.p);
  d.sse = reinterpret_cast<double*>(dv + o_sse);
  d.step = reinterpret_cast<double*>(dv + o_step);
  d.Sacc = reinterpret_cast<double*>(dv + o_S);
  d.racc = reinterpret_cast<double*>(dv + o_r);
  d.Lf = reinterpret_cast<double*>(dv + o_L);
  d.delta = reinterpret_cast<double*>(dv + o_delta);
  d.gauge = reinterpret_cast<double*>(dv + o_gauge);
  d.cov = reinterpret_cast<double*>(dv + o_cov);
  d.out = reinterpret_cast<double*>(dv + o_out);
  RigBaOutcome o;
  if (rig_ba_iterate(B, chunks, opt.max_iterations, opt.step_tolerance, o)) return fail(h, MPE_ERR_HIP, "mpe_body_calibrate", B.err);
  HIP_TRY(h, hipMemcpyAsync(mb + o_mk, dv + o_mk, (size_t)n_markers * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(mb + o_T, dv + o_T, (size_t)nv * 16 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(mb + o_cov, dv + o_cov, (size_t)nf * 9 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  B.read_out();
  const double* mk_back = reinterpret_cast<const double*>(mb + o_mk);
  const double* T_back = reinterpret_cast<const double*>(mb + o_T);
  const double* cov_back = reinterpret_cast<const double*>(mb + o_cov);
  return body_ba_hand_out(P, o, mk_back, T_back, cov_back, markers_out, T_view_out, cov_out, report);
}

int mpe_rig_calibration_start(const double* camera_pose, const int* updated, int n_views, int n_cameras,
                              int reference_camera, double* T_cam_rig_out, double* T_view_out, int* camera_linked) {
  if (!camera_pose || !updated || !T_cam_rig_out || !T_view_out || n_views < 0 || n_cameras < 1 ||
      n_cameras > MPE_RIG_MAX_CAMERAS || reference_camera < 0 || reference_camera >= n_cameras)
    return MPE_ERR_ARG;
  std::vector<M44> E((size_t)n_cameras, m44_identity());
  int round_of[MPE_RIG_MAX_CAMERAS];  // the round in which the camera was linked, -1 not yet
  for (int c = 0; c < n_cameras; ++c) round_of[c] = -1;
  round_of[reference_camera] = 0;
  auto pose = [&](int f, int c) { return m44_from(camera_pose + 16 * ((size_t)f * n_cameras + c)); };
  int n_linked = 1;
  for (int round = 1; round <= n_cameras; ++round) {
    bool any = false;
    for (int f = 0; f < n_views; ++f) {
      const int* u = updated + (size_t)f * n_cameras;
      int via = -1;  // the lowest camera linked in an earlier round that updated in f
      for (int c = 0; c < n_cameras && via < 0; ++c)
        if (u[c] && round_of[c] >= 0 && round_of[c] < round) via = c;
      if (via < 0) continue;
      for (int c = 0; c < n_cameras; ++c)
        if (u[c] && round_of[c] < 0) {
          E[(size_t)c] = m44_mul(m44_mul(pose(f, c), m44_rigid_inverse(pose(f, via))), E[(size_t)via]);
          round_of[c] = round;
          ++n_linked;
          any = true;
        }
    }
    if (!any) break;
  }
  for (int c = 0; c < n_cameras; ++c) {
    std::memcpy(T_cam_rig_out + 16 * (size_t)c, E[(size_t)c].a, 16 * sizeof(double));
    if (camera_linked) camera_linked[c] = round_of[c] >= 0 ? 1 : 0;
  }
  for (int f = 0; f < n_views; ++f) {
    M44 T = m44_identity();
    for (int c = 0; c < n_cameras; ++c)
      if (updated[(size_t)f * n_cameras + c] && round_of[c] >= 0) {
        T = m44_mul(m44_rigid_inverse(E[(size_t)c]), pose(f, c));
        break;
      }
    std::memcpy(T_view_out + 16 * (size_t)f, T.a, 16 * sizeof(double));
  }
  return n_linked;
}

}  // extern "C"
