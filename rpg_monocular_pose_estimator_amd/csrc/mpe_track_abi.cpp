// mpe_track_abi.cpp — host side of libmpe_hip.so, part 3 (see mpe_host.h): one tracked frame (mpe_track_step) and the
// lock-step time step of N camera streams (mpe_track_step_batch[_setups][_device[_encoded]][_submit / _collect / _cancel],
// mpe_track_step_batch_formats[_submit] for streams that differ in image size, stride and encoding); the
// per-stream state machine on top of them is mpe_tracker.cpp.  Every entry checks its own arguments and the image format
// it was given (check_image_format, mpe_pixel.h), describes where the pixels are and what they look like in one
// SlotPixels (mpe_host.h) and then makes the same submission (submit_tracked: the checks that need the items, then
// submit_slots): a uniform batch is the submission of one set-up and one format, a tracked frame a batch of one, and the
// description alone decides where the ROI slots come from — a host copy or one of three gather kernels.
#include "mpe_host.h"
#include "mpe_gather.h"

extern "C" {

namespace {
using clk = std::chrono::steady_clock;

// The records of n slots over one base pointer (device or pinned): n detection sets, n x 2*MPE_MAX_MARKERS
// correspondence words, n results
struct TrackRecords {
  mpe_detections* dets;
  uint32_t* corr;
  mpe_result* res;
  TrackRecords(void* base, int n)
      : dets(static_cast<mpe_detections*>(base)),
        corr(reinterpret_cast<uint32_t*>(dets + n)),
        res(reinterpret_cast<mpe_result*>(corr + (size_t)n * 2 * MPE_MAX_MARKERS)) {}
  static size_t bytes(int n) {
    return (size_t)n * (sizeof(mpe_detections) + 2 * MPE_MAX_MARKERS * sizeof(uint32_t) + sizeof(mpe_result));
  }
};

// ... and of a wide submission (mpe_track_step_batch_wide): n wide detection sets, n x 2*MPE_MAX_MARKERS correspondence
// words (indices into the compact record the tail ran on), n x MPE_MAX_MARKERS slot -> wide index words, n results
struct WideTrackRecords {
  mpe_detections_wide* dets;
  uint32_t* corr;
  uint32_t* slot;
  mpe_result* res;
  WideTrackRecords(void* base, int n)
      : dets(static_cast<mpe_detections_wide*>(base)),
        corr(reinterpret_cast<uint32_t*>(dets + n)),
        slot(corr + (size_t)n * 2 * MPE_MAX_MARKERS),
        res(reinterpret_cast<mpe_result*>(slot + (size_t)n * MPE_MAX_MARKERS)) {}
  static size_t bytes(int n) {
    return (size_t)n * (sizeof(mpe_detections_wide) + 3 * MPE_MAX_MARKERS * sizeof(uint32_t) + sizeof(mpe_result));
  }
};

bool roi_inside(const mpe_track_item& it, int rows, int cols) {
  return it.roi_x >= 0 && it.roi_y >= 0 && it.roi_w > 0 && it.roi_h > 0 && it.roi_x + it.roi_w <= cols &&
         it.roi_y + it.roi_h <= rows;
}

// the ROI of `it` into a g.rows x g.pitch slot, zero beyond it
void pack_roi(uint8_t* slot, const FrameGeom& g, const mpe_track_item& it, size_t stride_bytes) {
  for (int y = 0; y < g.rows; ++y) {
    uint8_t* dst = slot + (size_t)y * g.pitch;
    if (y < it.roi_h) {
      std::memcpy(dst, it.img + (size_t)(it.roi_y + y) * stride_bytes + it.roi_x, (size_t)it.roi_w);
      std::memset(dst + it.roi_w, 0, (size_t)(g.pitch - it.roi_w));
    } else {
      std::memset(dst, 0, (size_t)g.pitch);
    }
  }
}

// Every item's image must be a device allocation on the handle's device that holds the whole image: this check is what
// stands between a caller's mistake and a GPU fault.  Each distinct allocation is looked up once per call (the frames
// of N streams usually sit in one or a few).  (static, as prepare_setups below: inside extern "C" the unnamed namespace
// alone does not keep a name out of the library's exports, and these two are no part of them)
static int check_device_images(mpe_handle* h, const mpe_track_item* items, int n, const SlotPixels& px) {
  struct Span {
    uintptr_t lo, hi;
  };
  std::vector<Span> ok;
  for (int i = 0; i < n; ++i) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(items[i].img);
    const size_t img_bytes = image_extent(px.of(i));
    bool known = false;
    for (const Span& s : ok) known |= a >= s.lo && a + img_bytes <= s.hi;
    if (known) continue;
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, items[i].img) != hipSuccess) {
      (void)hipGetLastError();  // (an ordinary host pointer: the runtime reports it as an error)
      return fail(h, MPE_ERR_ARG, "img is not a device pointer (the host entries are for that)");
    }
    if (at.type != hipMemoryTypeDevice)
      return fail(h, MPE_ERR_ARG, "img is not a device allocation (the host entries are for that)");
    if (at.device != h->device) return fail(h, MPE_ERR_ARG, "img is on another device than the handle");
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<uint8_t*>(items[i].img)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(h, MPE_ERR_ARG, "img is not inside a device allocation");
    }
    const Span s = {reinterpret_cast<uintptr_t>(base), reinterpret_cast<uintptr_t>(base) + size};
    if (a < s.lo || a + img_bytes > s.hi) return fail(h, MPE_ERR_ARG, "the image reaches beyond its device allocation");
    ok.push_back(s);
  }
  return MPE_OK;
}

// the device workspaces of n slots of geometry g behind in_bytes of inputs
int reserve_track(mpe_handle* h, const FrameGeom& g, int n, size_t in_bytes) {
  HIP_TRY(h, h->frames.reserve(in_bytes + 16));
  HIP_TRY(h, h->flags.reserve(std::max(flag_words((size_t)n * g.rows * g.pitch), (size_t)n * track_flag_words(g)) * 8));
  HIP_TRY(h, h->work.reserve((size_t)2 * (n + 1) * sizeof(int)));
  HIP_TRY(h, h->scratch.reserve(k1b_scratch_bytes(g, n)));
  HIP_TRY(h, h->hist.reserve((size_t)n * MPE_HIST_STRIDE * sizeof(uint32_t)));
  HIP_TRY(h, h->track.reserve(TrackRecords::bytes(n)));
  HIP_TRY(h, h->mid.reserve(k3_mid_bytes(n)));
  return MPE_OK;
}
}  // namespace

int mpe_track_step(mpe_handle* h, const uint8_t* img, int rows, int cols, size_t stride_bytes, int roi_x, int roi_y,
                   int roi_w, int roi_h, const mpe_params* p, const double K[9], const double* D, int nD,
                   const double* markers_xyz, int n_markers, const double* predicted_px, mpe_detections* dets_out,
                   uint32_t* corr_out, mpe_result* out) {
  if (!h || !img || !p || !K || !markers_xyz || !predicted_px || !dets_out || !corr_out || !out)
    return fail(h, MPE_ERR_ARG, "bad argument");
  const mpe_track_item it = {img, roi_x, roi_y, roi_w, roi_h, predicted_px};
  if (!roi_inside(it, rows, cols)) return fail(h, MPE_ERR_ARG, "ROI outside the image");
  if (h->pending_track_n) return fail(h, MPE_ERR_ARG, "a submitted batch has not been collected yet (shared staging memory)");
  // a lock-step batch of one: its slot window gives the borders and centroid offsets of the ROI
  return mpe_track_step_batch(h, &it, 1, rows, cols, stride_bytes, p, K, D, nD, markers_xyz, n_markers, dets_out,
                              corr_out, out);
}

namespace {
// the chain of kernels over slot range r of the pending submission of n slots (scan, blob tiers — the small one alone
// when first_tier_only —, validate + refine), records to the device arrays
int track_range_chain(mpe_handle* h, const mpe_handle::PendingTrack::Range& r, int n, bool first_tier_only) {
  const mpe_handle::PendingTrack& pt = h->pending_track;
  const uint8_t* pix = pt.d_pix + (size_t)r.begin * pt.slot_bytes;
  const int* wins = static_cast<const int*>(pt.d_wins) + 4 * (size_t)r.begin;
  const TrackRecords d(h->track.p, n);
  unsigned long long* flags = static_cast<unsigned long long*>(h->flags.p);
  HIP_TRY(h, launch_k1a_scan(pix, (size_t)r.count * pt.slot_bytes, flags, r.su.dp.thr, 0, h->stream));
  HIP_TRY(h, launch_k1b_blobs(pix, flags, r.count, pt.g, r.su.dp, d.dets + r.begin, static_cast<int*>(h->work.p),
                              static_cast<uint8_t*>(h->scratch.p), h->scratch.cap, r.su.sp.n_markers, h->stream, wins,
                              false, first_tier_only));
  HIP_TRY(h, launch_k3_tail(d.dets + r.begin, static_cast<uint32_t*>(h->hist.p) + (size_t)r.begin * MPE_HIST_STRIDE,
                            r.count, r.su.sp, d.res + r.begin, d.corr + (size_t)r.begin * 2 * MPE_MAX_MARKERS, nullptr,
                            pt.d_pred + (size_t)r.begin * 2 * MPE_MAX_MARKERS, r.su.nn_tol, h->mid.p, h->stream));
  return MPE_OK;
}

// ---- lock-step batches: frame k of N independent camera streams in ONE device submission ---------------
// (BASELINE configs[4]: N streams' steps are independent of each other, pose_estimator.cpp:98-147 is sequential only
// within a stream.)  Every stream's ROI is cloned into one slot of a uniform slot array — zero beyond the ROI, the
// window size and origin in a per-slot table that the blob kernels read, so borders and centroid offsets are those
// of the stand-alone cv::Mat clone of led_detector.cpp:44.  Streams may differ in camera, marker set and parameters
// (one PoseEstimator per camera, pose_estimator.h:63,82-83, each filled from its own camera_info,
// monocular_pose_estimator.cpp:103-120): item i runs with setups[item_setup[i]] (item_setup null: set-up 0).  The slots
// are grouped by set-up, in stable order, the optimistic set-ups (1 .. 8 markers) first, so that every set-up occupies a
// contiguous range of slots and the fused ranges are a prefix: ONE launch of k_track_frame (scan, small blob tier,
// nearest-neighbour correspondences from the stream's predicted pixels, validate, refine) runs them, and every rare
// path (track_fused 0, set-ups of more than 8 markers, the re-run of a range that overflowed the small blob tier) is
// the chain of kernels over a range with its own parameters.  One copy brings the N records back; _collect un-permutes
// them.  The caller has checked the arguments and entered the handle.
// Where the pixels are is the one thing that varies, and px (SlotPixels, mpe_host.h) says it.  The slots are mono8
// whatever the source was, so nothing behind them, the overflow re-run in _collect included, knows the source:
//   host frames                          pack_roi with the item's own stride; the slots travel with the header
//   device frames, one format, mono8     the header carries a gather table, k_gather_rois writes the same slot bytes on
//                                        the device, in front of everything that reads them
//   device frames, one other format      k_gather_rois_encoded, which decodes what it gathers (stride and extent in
//                                        source bytes, the ROIs in pixels)
//   device frames, two or more formats   the header carries the format table behind the gather table and
//                                        k_gather_rois_formats decodes every item by its own entry
// An image ends with the last pixel of its last row (image_extent): the extent check_device_images has checked is the
// one every gather is given.  With two or more formats the slots of a set-up range are ordered by format (stable), so
// the gather's branch on the format diverges only in the waves that hold a slot boundary between two formats; with one
// format the slot order is that of the items.
// wide (mpe_track_step_batch_wide): the same slots, header and gather, nothing launched behind them — no range is fused,
// the header also carries one identity work-list per range for the general blob tier, the record area is sized for
// WideTrackRecords, and the submission is not left pending: run_wide_slots works it off synchronously.
int submit_slots(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n, const FrameGeom& g,
                 const TrackSetup* setups, int n_setups, const SlotPixels& px, bool wide) {
  const bool on_device = px.on_device, format_table = px.on_device && px.n_formats > 1;
  mpe_handle::PendingTrack& pt = h->pending_track;
  pt.t_in = h->track_profile ? clk::now() : clk::time_point();
  auto setup_of = [item_setup](int i) { return item_setup ? item_setup[i] : 0; };
  std::vector<int> count((size_t)n_setups, 0), range_of((size_t)n_setups, -1);
  for (int i = 0; i < n; ++i) ++count[(size_t)setup_of(i)];
  pt.ranges.clear();
  int n_fused = 0, fused_setups = 0, max_markers = 0;
  for (int pass = 0; pass < 2; ++pass)
    for (int s = 0; s < n_setups; ++s) {
      const bool opt = setups[s].sp.n_markers >= 1 && setups[s].sp.n_markers <= 8;
      if (!count[(size_t)s] || opt != (pass == 0)) continue;
      const int begin = pt.ranges.empty() ? 0 : pt.ranges.back().begin + pt.ranges.back().count;
      range_of[(size_t)s] = (int)pt.ranges.size();
      pt.ranges.push_back({begin, count[(size_t)s], opt, opt && h->track_fused != 0 && !wide, setups[s]});
      if (pt.ranges.back().fused) {
        n_fused += count[(size_t)s];
        ++fused_setups;
        max_markers = std::max(max_markers, setups[s].sp.n_markers);
      }
    }
  std::vector<int> fill(pt.ranges.size(), 0);
  pt.perm.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    const int r = range_of[(size_t)setup_of(i)];
    pt.perm[(size_t)(pt.ranges[(size_t)r].begin + fill[(size_t)r]++)] = i;
  }
  if (px.n_formats > 1)
    for (const mpe_handle::PendingTrack::Range& r : pt.ranges)
      std::stable_sort(pt.perm.begin() + r.begin, pt.perm.begin() + r.begin + r.count,
                       [&px](int a, int b) { return px.item_format[a] < px.item_format[b]; });
  // [predictions | windows | set-up table | slot -> set-up | work lists (wide) | gather table (device frames) | format
  // table (device frames of several formats) | ROI slots] in slot order; one H2D copy carries what the host has of it:
  // all of it, or the header in front of the slots.  The set-up table only for
  // a launch of two or more set-ups: one set-up goes as kernel arguments (the table instantiation is 5.6 % slower)
  const bool table = fused_setups >= 2;
  const size_t slot = (size_t)g.rows * g.pitch;
  const size_t pred_bytes = (size_t)n * 2 * MPE_MAX_MARKERS * sizeof(double);
  const size_t win_bytes = ((size_t)n * 4 * sizeof(int) + 15) & ~(size_t)15;
  const size_t tab_bytes = table ? (pt.ranges.size() * sizeof(TrackSetup) + 255) & ~(size_t)255 : 0;
  const size_t idx_bytes = table ? ((size_t)n * sizeof(int) + 15) & ~(size_t)15 : 0;
  const size_t list_off = pred_bytes + win_bytes + tab_bytes + idx_bytes;
  const size_t list_bytes = wide ? (((size_t)n + pt.ranges.size()) * sizeof(int) + 15) & ~(size_t)15 : 0;
  const size_t gat_off = list_off + list_bytes;
  const size_t fmt_off = gat_off + (on_device ? (size_t)n * sizeof(GatherItem) : 0);
  const size_t head_bytes =  // (a multiple of 16: the slots' alignment)
      fmt_off + (format_table ? (size_t)px.n_formats * sizeof(GatherFormat) : 0);
  const size_t in_bytes = head_bytes + (size_t)n * slot;
  const size_t staged_bytes = on_device ? head_bytes : in_bytes;
  const size_t rec_bytes = wide ? WideTrackRecords::bytes(n) : TrackRecords::bytes(n);
  int rc = grow_mailbox(h, staged_bytes + rec_bytes + 512);
  if (rc != MPE_OK) return rc;
  uint8_t* mb = static_cast<uint8_t*>(h->mailbox);
  double* pred = reinterpret_cast<double*>(mb);
  int* wins = reinterpret_cast<int*>(mb + pred_bytes);
  GatherItem* gat = reinterpret_cast<GatherItem*>(mb + gat_off);
  if (table) {
    TrackSetup* tab = reinterpret_cast<TrackSetup*>(mb + pred_bytes + win_bytes);
    int* slot_setup = reinterpret_cast<int*>(mb + pred_bytes + win_bytes + tab_bytes);
    for (size_t r = 0; r < pt.ranges.size(); ++r) {
      tab[r] = pt.ranges[r].su;
      for (int k = pt.ranges[r].begin; k < pt.ranges[r].begin + pt.ranges[r].count; ++k) slot_setup[k] = (int)r;
    }
  }
  if (wide) {  // range r's list: its count, then its slots relative to its first one
    int* list = reinterpret_cast<int*>(mb + list_off);
    for (const mpe_handle::PendingTrack::Range& r : pt.ranges) {
      *list++ = r.count;
      for (int k = 0; k < r.count; ++k) *list++ = k;
    }
  }
  const double qnan = std::nan("");
  bool sensor_formats = false;  // an item of the format table is a YUV or a Bayer image
  for (int k = 0; k < n; ++k) {
    const int i = pt.perm[(size_t)k];
    const mpe_track_item& it = items[i];
    const int nm = setups[setup_of(i)].sp.n_markers;
    // no predicted pixels = detection only: NaN predictions are nearest to nothing, the tail then reports "no pose"
    for (int q = 0; q < 2 * MPE_MAX_MARKERS; ++q)
      pred[(size_t)k * 2 * MPE_MAX_MARKERS + q] = !it.predicted_px ? qnan : (q < 2 * nm ? it.predicted_px[q] : 0.0);
    wins[4 * k] = it.roi_h;
    wins[4 * k + 1] = it.roi_w;
    wins[4 * k + 2] = it.roi_x;
    wins[4 * k + 3] = it.roi_y;
    if (on_device)
      gat[k] = GatherItem{it.img, it.roi_x, it.roi_y, it.roi_w, it.roi_h, k, px.item_format ? px.item_format[i] : 0};
    else
      pack_roi(mb + head_bytes + (size_t)k * slot, g, it, px.of(i).stride_bytes);
    if (format_table) sensor_formats |= encoding_kind(px.of(i).encoding) != PIX_PLAIN;
  }
  if (format_table) {
    GatherFormat* tab = reinterpret_cast<GatherFormat*>(mb + fmt_off);
    for (int f = 0; f < px.n_formats; ++f) {
      const mpe_image_format& mf = px.formats[f];
      const int kind = encoding_kind(mf.encoding);
      tab[f] = GatherFormat{(uint64_t)mf.stride_bytes, (uint64_t)image_extent(mf), encoding_bytes_per_pixel(mf.encoding),
                            mf.encoding == MPE_ENC_RGB8 || mf.encoding == MPE_ENC_RGBA8,
                            mf.encoding == MPE_ENC_MONO16 && mf.src_big_endian, kind};
      if (kind == PIX_YUV) tab[f].big_endian = yuv_y_byte(mf.encoding);
      if (kind == PIX_BAYER) {  // (the neighbourhood decode clamps at the image's edges: its size, and the pattern)
        tab[f].rgb = mf.cols;
        tab[f].big_endian = mf.rows;
        tab[f].kind = PIX_BAYER | (bayer_phase(mf.encoding) << 8);
      }
    }
  }
  uint8_t* host_rec = mb + ((staged_bytes + 255) & ~(size_t)255);
  if ((rc = reserve_track(h, g, n, in_bytes)) != MPE_OK) return rc;
  if (wide) {  // (the compact records and rows k_nn_wide hands to the tail stay on the device)
    HIP_TRY(h, h->track.reserve(rec_bytes));
    HIP_TRY(h, h->dets.reserve((size_t)n * sizeof(mpe_detections)));
    HIP_TRY(h, h->corr.reserve((size_t)n * 2 * MPE_MAX_MARKERS * sizeof(uint32_t)));
  }
  uint8_t* d_in = static_cast<uint8_t*>(h->frames.p);
  h->have_ms = false;
  if (h->track_profile) pt.t_packed = clk::now();
  // (Zero-copy I/O — the kernels reading the pinned mailbox over PCIe, a copy kernel writing the record back — was
  //  built and measured in round 3: the image scan then waits for PCIe reads (4 -> 46 us for 64 streams) and the step
  //  is no faster, 0.135 vs 0.136 ms for one stream.  The two copy commands stay.)
  HIP_TRY(h, hipMemcpyAsync(d_in, mb, staged_bytes, hipMemcpyHostToDevice, h->stream));
  pt.g = g;
  pt.slot_bytes = slot;
  pt.rec_bytes = rec_bytes;
  pt.d_pred = reinterpret_cast<const double*>(d_in);
  pt.d_wins = d_in + pred_bytes;
  pt.d_pix = d_in + head_bytes;
  pt.d_list = reinterpret_cast<const int*>(d_in + list_off);
  const GatherItem* d_gat = reinterpret_cast<const GatherItem*>(d_in + gat_off);
  const mpe_image_format& f0 = px.formats[0];
  if (format_table)
    HIP_TRY(h, launch_gather_rois_formats(d_gat, reinterpret_cast<const GatherFormat*>(d_in + fmt_off), n, d_in + head_bytes, g,
                                          sensor_formats, h->stream));
  else if (on_device && f0.encoding == MPE_ENC_MONO8)
    HIP_TRY(h, launch_gather_rois(d_gat, n, d_in + head_bytes, g, f0.stride_bytes, image_extent(f0), h->stream));
  else if (on_device)
    HIP_TRY(h, launch_gather_rois_encoded(d_gat, n, d_in + head_bytes, g, f0.stride_bytes, image_extent(f0), f0.encoding,
                                          f0.src_big_endian ? 1 : 0, h->stream));
  if (wide) {
    h->pending_track_rec = host_rec;  // (for run_wide_slots, which follows at once: nothing stays pending)
    return MPE_OK;
  }
  ++h->track_batch_submits;
  // round 6: the fused ranges as ONE launch, a block per stream (k_track_frame), the records stored to the pinned
  // staging memory by the kernel (track_fused 2) — scan, small blob tier, tail and copy-out were five commands, and
  // every stage waited for the slowest stream of the one before
  const bool deliver = h->track_fused >= 2;
  if (n_fused) {
    const TrackRecords d(h->track.p, n), hr(host_rec, n);
    TrackFramesArgs ta = {pt.d_pix, slot, pt.d_pred, pt.d_wins, static_cast<unsigned long long*>(h->flags.p),
                          static_cast<uint32_t*>(h->hist.p), h->mid.p, d.dets, d.corr, d.res, deliver ? hr.dets : nullptr,
                          deliver ? hr.corr : nullptr, deliver ? hr.res : nullptr, h->track_clk};
    const TrackSetup& su = pt.ranges[0].su;
    if (!table)
      HIP_TRY(h, launch_track_frames(ta, n_fused, g, su.dp, su.sp, su.nn_tol, h->stream));
    else
      HIP_TRY(h, launch_track_frames_setups(ta, n_fused, g, reinterpret_cast<const TrackSetup*>(d_in + pred_bytes + win_bytes),
                                            reinterpret_cast<const int*>(d_in + pred_bytes + win_bytes + tab_bytes),
                                            max_markers, h->stream));
  }
  // the rest (track_fused 0, set-ups of more than 8 markers): the chain of kernels per set-up
  for (const mpe_handle::PendingTrack::Range& r : pt.ranges) {
    if (r.fused) continue;
    if ((rc = track_range_chain(h, r, n, r.optimistic)) != MPE_OK) return rc;
    ++h->track_batch_chains;
  }
  if (n_fused < n || !deliver) HIP_TRY(h, hipMemcpyAsync(host_rec, h->track.p, rec_bytes, hipMemcpyDeviceToHost, h->stream));
  if (h->track_profile) pt.t_queued = clk::now();
  h->pending_track_n = n;
  h->pending_track_rec = host_rec;
  return MPE_OK;
}

// The usage errors of a submission that need its items, every one before any device work: no submission in flight, the
// set-ups, every item's set-up index (item_setup null: set-up 0) and its ROI against its own format; then the slot
// geometry g and the prepared parameters of the set-ups that have streams.  n == 0: MPE_OK with nothing prepared — there
// is nothing to submit.
static int prepare_setups(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n,
                          const mpe_track_setup* setups, int n_setups, const SlotPixels& px, FrameGeom& g,
                          std::vector<TrackSetup>& prep) {
  if (h->pending_track_n) return fail(h, MPE_ERR_ARG, "a submitted batch has not been collected yet");
  for (int s = 0; s < n_setups; ++s) {
    const mpe_track_setup& su = setups[s];
    if (!su.p || !su.K || !su.markers_xyz || su.nD < 0 || (su.nD > 0 && !su.D))
      return fail(h, MPE_ERR_ARG, "bad set-up");
    if (su.n_markers < 0 || su.n_markers > MPE_MAX_MARKERS) return fail(h, MPE_ERR_ARG, "set-up with n_markers > MPE_MAX_MARKERS");
  }
  int rmax = 0, wmax = 0;
  std::vector<char> used((size_t)n_setups, 0);
  for (int i = 0; i < n; ++i) {
    const int s = item_setup ? item_setup[i] : 0;
    if (s < 0 || s >= n_setups) return fail(h, MPE_ERR_ARG, "set-up index out of range");
    if (!items[i].img || !roi_inside(items[i], px.of(i).rows, px.of(i).cols))
      return fail(h, MPE_ERR_ARG, "ROI outside the image");
    used[(size_t)s] = 1;
    rmax = std::max(rmax, items[i].roi_h);
    wmax = std::max(wmax, items[i].roi_w);
  }
  if (n == 0) return MPE_OK;
  if (make_geom(h, rmax, wmax, g)) return fail(h, MPE_ERR_UNSUPPORTED, "frame size unsupported");
  prep = std::vector<TrackSetup>((size_t)n_setups);
  for (int s = 0; s < n_setups; ++s) {  // (the set-ups that have streams)
    const mpe_track_setup& su = setups[s];
    if (!used[(size_t)s]) continue;
    if (make_detect_params(su.p, su.K, su.D, su.nD, 0, 0, prep[(size_t)s].dp)) return fail(h, MPE_ERR_ARG, "gaussian_sigma must be in (0, 6]");
    if (make_solve_params(h, su.p, su.markers_xyz, su.n_markers, su.K, prep[(size_t)s].sp)) return fail(h, MPE_ERR_ARG, "bad set-up");
    prep[(size_t)s].nn_tol = su.p->nearest_neighbour_pixel_tolerance;
  }
  return MPE_OK;
}
}  // namespace

}  // extern "C"

int mpe_host::submit_tracked(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n,
                             const mpe_track_setup* setups, int n_setups, const SlotPixels& px, bool wide) {
  FrameGeom g;
  std::vector<TrackSetup> prep;
  int rc = prepare_setups(h, items, item_setup, n, setups, n_setups, px, g, prep);
  if (rc != MPE_OK || n == 0) return rc;
  ENTER(h);
  if (px.on_device && (rc = check_device_images(h, items, n, px)) != MPE_OK) return rc;
  return submit_slots(h, items, item_setup, n, g, prep.data(), n_setups, px, wide);
}

extern "C" {

// (the one entry that takes its set-up as plain arguments, and answers for it with codes of its own)
int mpe_track_step_batch_submit(mpe_handle* h, const mpe_track_item* items, int n, int rows, int cols,
                                size_t stride_bytes, const mpe_params* p, const double K[9], const double* D, int nD,
                                const double* markers_xyz, int n_markers) {
  if (!h || !items || n < 0 || !p || !K || !markers_xyz) return fail(h, MPE_ERR_ARG, "bad argument");
  if (h->pending_track_n) return fail(h, MPE_ERR_ARG, "a submitted batch has not been collected yet");
  if (n == 0) return MPE_OK;
  int rmax = 0, wmax = 0;
  for (int i = 0; i < n; ++i) {
    if (!items[i].img || !roi_inside(items[i], rows, cols)) return fail(h, MPE_ERR_ARG, "ROI outside the image");
    rmax = std::max(rmax, items[i].roi_h);
    wmax = std::max(wmax, items[i].roi_w);
  }
  ENTER(h);
  FrameGeom g;
  if (make_geom(h, rmax, wmax, g)) return fail(h, MPE_ERR_UNSUPPORTED, "frame size unsupported");
  TrackSetup su;
  if (make_detect_params(p, K, D, nD, 0, 0, su.dp)) return fail(h, MPE_ERR_ARG, "gaussian_sigma must be in (0, 6]");
  if (make_solve_params(h, p, markers_xyz, n_markers, K, su.sp)) return fail(h, MPE_ERR_UNSUPPORTED, "n_markers > MPE_MAX_MARKERS");
  su.nn_tol = p->nearest_neighbour_pixel_tolerance;
  const mpe_image_format f = {rows, cols, stride_bytes, MPE_ENC_MONO8, 0};
  return submit_slots(h, items, nullptr, n, g, &su, 1, SlotPixels{false, nullptr, &f, 1}, false);
}

int mpe_track_step_batch_setups_submit(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n, int rows,
                                       int cols, size_t stride_bytes, const mpe_track_setup* setups, int n_setups) {
  // every usage error before any device work
  if (!h || !items || !item_setup || n < 0 || !setups || n_setups < 1) return fail(h, MPE_ERR_ARG, "bad argument");
  // (host frames are mono8 by this entry's signature; a size that holds no pixels fails as a ROI outside the image)
  const mpe_image_format f = {rows, cols, stride_bytes, MPE_ENC_MONO8, 0};
  return submit_tracked(h, items, item_setup, n, setups, n_setups, SlotPixels{false, nullptr, &f, 1}, false);
}

int mpe_track_step_batch_setups_device_submit(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n,
                                              int rows, int cols, size_t stride_bytes, const mpe_track_setup* setups,
                                              int n_setups) {
  // every usage error before any device work, with the codes and messages of mpe_track_step_batch_setups_submit
  if (!h || !items || n < 0 || !setups || n_setups < 1 || (!item_setup && n_setups != 1) || rows < 1 || cols < 1 ||
      stride_bytes < (size_t)cols)
    return fail(h, MPE_ERR_ARG, "bad argument");
  const mpe_image_format f = {rows, cols, stride_bytes, MPE_ENC_MONO8, 0};
  return submit_tracked(h, items, item_setup, n, setups, n_setups, SlotPixels{true, nullptr, &f, 1}, false);
}

int mpe_track_step_batch_setups_device(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n, int rows,
                                       int cols, size_t stride_bytes, const mpe_track_setup* setups, int n_setups,
                                       mpe_detections* dets_out, uint32_t* corr_out, mpe_result* out) {
  if (!dets_out || !corr_out || !out) return fail(h, MPE_ERR_ARG, "bad argument");
  const int rc = mpe_track_step_batch_setups_device_submit(h, items, item_setup, n, rows, cols, stride_bytes, setups, n_setups);
  if (rc != MPE_OK) return rc;
  if (n == 0) return MPE_OK;  // (nothing was submitted)
  return mpe_track_step_batch_collect(h, dets_out, corr_out, out);
}

int mpe_track_step_batch_setups_device_encoded_submit(mpe_handle* h, const mpe_track_item* items, const int* item_setup,
                                                      int n, int rows, int cols, size_t stride_bytes, int encoding,
                                                      int src_big_endian, const mpe_track_setup* setups, int n_setups) {
  // every usage error before any device work: those of mpe_track_step_batch_setups_device_submit, and the encoding
  if (!h || !items || n < 0 || !setups || n_setups < 1 || (!item_setup && n_setups != 1) || rows < 1 || cols < 1)
    return fail(h, MPE_ERR_ARG, "bad argument");
  const mpe_image_format f = {rows, cols, stride_bytes, encoding, src_big_endian};
  const FormatRefusal no = check_image_format(f, true);
  if (no.code != MPE_OK) return fail(h, no.code, no.msg);
  // (MPE_ENC_MONO8: nothing to decode — the submission of mpe_track_step_batch_setups_device_submit, and k_gather_rois)
  return submit_tracked(h, items, item_setup, n, setups, n_setups, SlotPixels{true, nullptr, &f, 1}, false);
}

int mpe_track_step_batch_setups_device_encoded(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n,
                                               int rows, int cols, size_t stride_bytes, int encoding, int src_big_endian,
                                               const mpe_track_setup* setups, int n_setups, mpe_detections* dets_out,
                                               uint32_t* corr_out, mpe_result* out) {
  if (!dets_out || !corr_out || !out) return fail(h, MPE_ERR_ARG, "bad argument");
  const int rc = mpe_track_step_batch_setups_device_encoded_submit(h, items, item_setup, n, rows, cols, stride_bytes, encoding,
                                                                   src_big_endian, setups, n_setups);
  if (rc != MPE_OK) return rc;
  if (n == 0) return MPE_OK;  // (nothing was submitted)
  return mpe_track_step_batch_collect(h, dets_out, corr_out, out);
}

int mpe_track_step_batch_formats_submit(mpe_handle* h, const mpe_track_item* items, const int* item_setup,
                                        const int* item_format, int n, const mpe_image_format* formats, int n_formats,
                                        int frames_on_device, const mpe_track_setup* setups, int n_setups) {
  // every usage error before any device work
  if (!h || !items || n < 0 || !setups || n_setups < 1 || (!item_setup && n_setups != 1) || !formats || n_formats < 1 ||
      (!item_format && n_formats != 1))
    return fail(h, MPE_ERR_ARG, "bad argument");
  for (int f = 0; f < n_formats; ++f) {
    const FormatRefusal no = check_format_shape(formats[f], frames_on_device != 0);
    if (no.code != MPE_OK) return fail(h, no.code, no.msg);
  }
  // the distinct formats that have items, in order of first use, and every item's index among them
  std::vector<mpe_image_format> used;
  std::vector<int> dense((size_t)n_formats, -1), item_dense((size_t)n);
  for (int i = 0; i < n; ++i) {
    const int f = item_format ? item_format[i] : 0;
    if (f < 0 || f >= n_formats) return fail(h, MPE_ERR_ARG, "format index out of range");
    if (dense[(size_t)f] < 0) {
      const FormatRefusal no = check_image_format(formats[f], frames_on_device != 0);  // (now that it has an item)
      if (no.code != MPE_OK) return fail(h, no.code, no.msg);
      size_t k = 0;
      while (k < used.size() && !same_image_format(used[k], formats[f])) ++k;
      if (k == used.size()) used.push_back(formats[f]);
      dense[(size_t)f] = (int)k;
    }
    item_dense[(size_t)i] = dense[(size_t)f];
  }
  // (one distinct format: the gather and the records of that format's own entry)
  const SlotPixels px = {frames_on_device != 0, item_dense.data(), used.data(), (int)used.size()};
  return submit_tracked(h, items, item_setup, n, setups, n_setups, px, false);
}

int mpe_track_step_batch_formats(mpe_handle* h, const mpe_track_item* items, const int* item_setup, const int* item_format,
                                 int n, const mpe_image_format* formats, int n_formats, int frames_on_device,
                                 const mpe_track_setup* setups, int n_setups, mpe_detections* dets_out, uint32_t* corr_out,
                                 mpe_result* out) {
  if (!dets_out || !corr_out || !out) return fail(h, MPE_ERR_ARG, "bad argument");
  const int rc = mpe_track_step_batch_formats_submit(h, items, item_setup, item_format, n, formats, n_formats,
                                                     frames_on_device, setups, n_setups);
  if (rc != MPE_OK) return rc;
  if (n == 0) return MPE_OK;  // (nothing was submitted)
  return mpe_track_step_batch_collect(h, dets_out, corr_out, out);
}

int mpe_track_step_batch_setups(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n, int rows, int cols,
                                size_t stride_bytes, const mpe_track_setup* setups, int n_setups, mpe_detections* dets_out,
                                uint32_t* corr_out, mpe_result* out) {
  if (!dets_out || !corr_out || !out) return fail(h, MPE_ERR_ARG, "bad argument");
  const int rc = mpe_track_step_batch_setups_submit(h, items, item_setup, n, rows, cols, stride_bytes, setups, n_setups);
  if (rc != MPE_OK) return rc;
  if (n == 0) return MPE_OK;  // (nothing was submitted)
  return mpe_track_step_batch_collect(h, dets_out, corr_out, out);
}

namespace {
// The wide submission submit_slots has staged (wide = true), worked off: per set-up range the image scan, the general
// blob tier with the wide writer and the slot windows, k_nn_wide (correspondences from the predicted pixels, compact
// record + rows) and the tail with given rows; one copy back, rows mapped back to wide indices, items un-permuted.
static int run_wide_slots(mpe_handle* h, int n, mpe_detections_wide* dets_out, uint32_t* corr_out, mpe_result* out) {
  const mpe_handle::PendingTrack& pt = h->pending_track;
  uint8_t* host_rec = h->pending_track_rec;
  h->pending_track_rec = nullptr;
  const WideTrackRecords d(h->track.p, n), rec(host_rec, n);
  unsigned long long* flags = static_cast<unsigned long long*>(h->flags.p);
  mpe_detections* compact = static_cast<mpe_detections*>(h->dets.p);
  uint32_t* rows_in = static_cast<uint32_t*>(h->corr.p);
  ++h->wide_track_submits;
  size_t ri = 0;
  for (const mpe_handle::PendingTrack::Range& r : pt.ranges) {
    const uint8_t* pix = pt.d_pix + (size_t)r.begin * pt.slot_bytes;
    const int* wins = static_cast<const int*>(pt.d_wins) + 4 * (size_t)r.begin;
    const size_t c0 = (size_t)r.begin * 2 * MPE_MAX_MARKERS;
    HIP_TRY(h, launch_k1a_scan(pix, (size_t)r.count * pt.slot_bytes, flags, r.su.dp.thr, 0, h->stream));
    HIP_TRY(h, launch_k1b_general_wide(pix, flags, r.count, pt.g, r.su.dp, d.dets + r.begin, pt.d_list + r.begin + ri,
                                       static_cast<uint8_t*>(h->scratch.p), h->scratch.cap, h->stream, h->general_lds == 1,
                                       wins));
    HIP_TRY(h, launch_k_nn_wide(d.dets + r.begin, pt.d_pred + c0, r.count, r.su.sp.n_markers, r.su.nn_tol,
                                compact + r.begin, rows_in + c0, d.slot + (size_t)r.begin * MPE_MAX_MARKERS, h->stream));
    // (the validation kernel takes its rows from rows_in and never reads a histogram: the pointer is only offset)
    HIP_TRY(h, launch_k3_tail(compact + r.begin, static_cast<uint32_t*>(h->hist.p), r.count, r.su.sp, d.res + r.begin,
                              d.corr + c0, rows_in + c0, nullptr, 0.0, h->mid.p, h->stream, 0));
    ++ri;
  }
  HIP_TRY(h, hipMemcpyAsync(host_rec, h->track.p, pt.rec_bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < n; ++k) {  // slot k -> the caller's item perm[k]
    const int i = pt.perm[(size_t)k];
    dets_out[i] = rec.dets[k];
    out[i] = rec.res[k];
    out[i].n_det = rec.dets[k].n;
    uint32_t* co = corr_out + (size_t)i * 2 * MPE_MAX_MARKERS;
    const uint32_t* ci = rec.corr + (size_t)k * 2 * MPE_MAX_MARKERS;
    std::memset(co, 0, 2 * MPE_MAX_MARKERS * sizeof(uint32_t));
    for (int r = 0; r < out[i].n_corr && r < MPE_MAX_MARKERS; ++r) {
      const uint32_t s = ci[2 * r + 1];
      co[2 * r] = ci[2 * r];
      co[2 * r + 1] = (s >= 1 && s <= MPE_MAX_MARKERS) ? rec.slot[(size_t)k * MPE_MAX_MARKERS + (s - 1)] : 0u;
    }
  }
  return MPE_OK;
}
}  // namespace

int mpe_track_step_batch_wide(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n, int rows, int cols,
                              size_t stride_bytes, int frames_on_device, int encoding, int src_big_endian,
                              const mpe_track_setup* setups, int n_setups, mpe_detections_wide* dets_out,
                              uint32_t* corr_out, mpe_result* out) {
  // every usage error before any device work: those of the narrow entries of the same source
  if (!h || !items || n < 0 || !setups || n_setups < 1 || (!item_setup && n_setups != 1) || rows < 1 || cols < 1 ||
      !dets_out || !corr_out || !out)
    return fail(h, MPE_ERR_ARG, "bad argument");
  const mpe_image_format f = {rows, cols, stride_bytes, encoding, src_big_endian};
  // (this entry has always named the host rule before the stride: the three rules in its own order)
  FormatRefusal no = refuse_encoding(encoding, frames_on_device != 0);
  if (no.code == MPE_OK) no = refuse_host_encoding(encoding, frames_on_device != 0);
  if (no.code == MPE_OK) no = refuse_size(f);
  if (no.code != MPE_OK) return fail(h, no.code, no.msg);
  if (h->submit_seq != h->collect_seq) return fail(h, MPE_ERR_ARG, "a submitted batch has not been collected yet");
  const int rc = submit_tracked(h, items, item_setup, n, setups, n_setups, SlotPixels{frames_on_device != 0, nullptr, &f, 1}, true);
  if (rc != MPE_OK || n == 0) return rc;
  return run_wide_slots(h, n, dets_out, corr_out, out);
}

int mpe_track_step_batch_cancel(mpe_handle* h) {
  if (!h) return MPE_ERR_ARG;
  if (h->pending_track_n == 0) return MPE_OK;
  h->pending_track_n = 0;
  h->pending_track_rec = nullptr;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // the copy-out of the abandoned submission has left the staging memory
  return MPE_OK;
}

int mpe_track_step_batch_collect(mpe_handle* h, mpe_detections* dets_out, uint32_t* corr_out, mpe_result* out) {
  if (!h || !dets_out || !corr_out || !out) return fail(h, MPE_ERR_ARG, "bad argument");
  const int n = h->pending_track_n;
  if (n == 0) return fail(h, MPE_ERR_ARG, "no submitted batch to collect (did mpe_track_step_batch_submit fail?)");
  uint8_t* host_rec = h->pending_track_rec;
  h->pending_track_n = 0;
  h->pending_track_rec = nullptr;
  ENTER(h);
  // (polling hipStreamQuery instead of blocking in the runtime's wait measured 133-135 against 128-129 us per frame)
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  const mpe_handle::PendingTrack& pt = h->pending_track;
  const TrackRecords rec(host_rec, n);
  // option "track_phase_clocks": the stamps of block 0 = slot 0, unless that frame is repeated below
  if (h->track_clk && pt.ranges[0].fused && rec.dets[0].status != MPE_FRAME_TOO_MANY_ROWS) {
    for (int i = 0; i < 4; ++i) h->track_clk_sum[i] += h->track_clk[i + 1] - h->track_clk[i];
    ++h->track_clk_n;
  }
  // a slot that overflowed the small blob tier: its set-up's range again, through every tier (the inputs are still on
  // the device: nothing has been submitted on this handle since)
  bool again = false;
  for (const mpe_handle::PendingTrack::Range& r : pt.ranges) {
    if (!r.optimistic) continue;
    bool over = false;
    for (int k = r.begin; k < r.begin + r.count && !over; ++k) over = rec.dets[k].status == MPE_FRAME_TOO_MANY_ROWS;
    if (!over) continue;
    const int rc = track_range_chain(h, r, n, false);
    if (rc != MPE_OK) return rc;
    ++h->track_batch_reruns;
    again = true;
  }
  if (again) {
    HIP_TRY(h, hipMemcpyAsync(host_rec, h->track.p, pt.rec_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  if (h->track_profile && pt.t_in != clk::time_point()) {  // (a submission made before the option was set: untimed)
    auto ns = [](clk::time_point a, clk::time_point b) { return (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count(); };
    h->track_ns[0] += ns(pt.t_in, pt.t_packed);
    h->track_ns[1] += ns(pt.t_packed, pt.t_queued);
    h->track_ns[2] += ns(pt.t_queued, clk::now());
    ++h->track_steps;
  }
  // slot k holds item k (always so with one set-up): one copy per array — slot by slot, a time step of 64 uniform streams
  // measured 5 us longer
  if (std::is_sorted(pt.perm.begin(), pt.perm.end())) {
    std::memcpy(dets_out, rec.dets, (size_t)n * sizeof(mpe_detections));
    std::memcpy(corr_out, rec.corr, (size_t)n * 2 * MPE_MAX_MARKERS * sizeof(uint32_t));
    std::memcpy(out, rec.res, (size_t)n * sizeof(mpe_result));
    return MPE_OK;
  }
  for (int k = 0; k < n; ++k) {  // slot k -> the caller's item perm[k]
    const int i = pt.perm[(size_t)k];
    dets_out[i] = rec.dets[k];
    std::memcpy(corr_out + (size_t)i * 2 * MPE_MAX_MARKERS, rec.corr + (size_t)k * 2 * MPE_MAX_MARKERS,
                2 * MPE_MAX_MARKERS * sizeof(uint32_t));
    out[i] = rec.res[k];
  }
  return MPE_OK;
}

int mpe_track_step_batch(mpe_handle* h, const mpe_track_item* items, int n, int rows, int cols, size_t stride_bytes,
                         const mpe_params* p, const double K[9], const double* D, int nD, const double* markers_xyz,
                         int n_markers, mpe_detections* dets_out, uint32_t* corr_out, mpe_result* out) {
  if (!dets_out || !corr_out || !out) return fail(h, MPE_ERR_ARG, "bad argument");
  const int rc = mpe_track_step_batch_submit(h, items, n, rows, cols, stride_bytes, p, K, D, nD, markers_xyz, n_markers);
  if (rc != MPE_OK) return rc;
  if (n == 0) return MPE_OK;  // (nothing was submitted)
  return mpe_track_step_batch_collect(h, dets_out, corr_out, out);
}

}  // extern "C"
