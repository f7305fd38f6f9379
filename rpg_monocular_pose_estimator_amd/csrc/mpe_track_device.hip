// mpe_track_device.hip — the lock-step time step of N camera streams whose frames are in DEVICE memory
// (mpe_track_step_batch_setups_device[_submit]): the submission of mpe_track_abi.cpp (submit_slots) with one
// difference — the ROI slots are not packed on the host and copied, a gather kernel (k_gather_rois) writes them from
// the caller's device images.  The slot bytes are those pack_roi writes, everything behind them is the same sequence of
// launches on the same buffers, so the records are those of the host-frame entries and mpe_track_step_batch_collect /
// _cancel serve this submission unchanged.
#include "mpe_host.h"
#include "mpe_gather.h"

namespace {

// ---- device side -----------------------------------------------------------------------------------------------------
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

hipError_t launch_gather_rois(const GatherItem* tab, int n, uint8_t* dst, const FrameGeom& g, size_t stride, size_t img_bytes,
                              hipStream_t s) {
  const size_t total = (size_t)n * g.rows * g.segs_per_row;
  const size_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gather_rois, dim3((unsigned)blocks), dim3(256), 0, s, tab, n, dst, (size_t)g.rows * g.pitch, g.rows,
                     g.segs_per_row, stride, img_bytes);
  return hipGetLastError();
}

// ---- host side -------------------------------------------------------------------------------------------------------
// TrackRecords, roi_inside, grow_mailbox, reserve_track and track_range_chain restate their namesakes in
// mpe_track_abi.cpp, and submit_device_slots restates submit_slots: those live in an anonymous namespace of a file whose
// bytes are part of source_fingerprint(), which ties the committed counter collection to the sources — sharing them
// means collecting the counters again.  Whoever next re-collects the profiles folds both submissions into one routine
// with a pixel-source parameter.  Until then: a change to the layout there is a change here.
using clk = std::chrono::steady_clock;

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

bool roi_inside(const mpe_track_item& it, int rows, int cols) {
  return it.roi_x >= 0 && it.roi_y >= 0 && it.roi_w > 0 && it.roi_h > 0 && it.roi_x + it.roi_w <= cols &&
         it.roi_y + it.roi_h <= rows;
}

int grow_mailbox(mpe_handle* h, size_t need) {
  if (need <= h->mailbox_cap) return MPE_OK;
  if (h->mailbox) (void)hipHostFree(h->mailbox);
  h->mailbox = nullptr;
  h->mailbox_cap = 0;
  const size_t want = std::max(need + need / 4, (size_t)1 << 16);
  HIP_TRY(h, hipHostMalloc(&h->mailbox, want, hipHostMallocDefault));
  h->mailbox_cap = want;
  return MPE_OK;
}

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

// Every item's image must be a device allocation on the handle's device that holds the whole image: this check is what
// stands between a caller's mistake and a GPU fault.  Each distinct allocation is looked up once per call (the frames
// of N streams usually sit in one or a few).
int check_device_images(mpe_handle* h, const mpe_track_item* items, int n, size_t img_bytes) {
  struct Span {
    uintptr_t lo, hi;
  };
  std::vector<Span> ok;
  for (int i = 0; i < n; ++i) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(items[i].img);
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

// submit_slots of mpe_track_abi.cpp with the slots gathered on the device: [predictions | windows | set-up table |
// slot -> set-up | gather table] is what the one H2D copy carries, the slots follow on the device.  cols: image width
// (the image ends with the last pixel of its last row).
int submit_device_slots(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n, const FrameGeom& g,
                        size_t stride_bytes, size_t img_bytes, const TrackSetup* setups, int n_setups) {
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
      pt.ranges.push_back({begin, count[(size_t)s], opt, opt && h->track_fused != 0, setups[s]});
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
  const bool table = fused_setups >= 2;
  const size_t slot = (size_t)g.rows * g.pitch;
  const size_t pred_bytes = (size_t)n * 2 * MPE_MAX_MARKERS * sizeof(double);
  const size_t win_bytes = ((size_t)n * 4 * sizeof(int) + 15) & ~(size_t)15;
  const size_t tab_bytes = table ? (pt.ranges.size() * sizeof(TrackSetup) + 255) & ~(size_t)255 : 0;
  const size_t idx_bytes = table ? ((size_t)n * sizeof(int) + 15) & ~(size_t)15 : 0;
  const size_t gat_off = pred_bytes + win_bytes + tab_bytes + idx_bytes;
  const size_t head_bytes = gat_off + (size_t)n * sizeof(GatherItem);  // (a multiple of 16: the slots' alignment)
  const size_t in_bytes = head_bytes + (size_t)n * slot;
  const size_t rec_bytes = TrackRecords::bytes(n);
  int rc = grow_mailbox(h, head_bytes + rec_bytes + 512);
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
  const double qnan = std::nan("");
  for (int k = 0; k < n; ++k) {
    const int i = pt.perm[(size_t)k];
    const mpe_track_item& it = items[i];
    const int nm = setups[setup_of(i)].sp.n_markers;
    for (int q = 0; q < 2 * MPE_MAX_MARKERS; ++q)
      pred[(size_t)k * 2 * MPE_MAX_MARKERS + q] = !it.predicted_px ? qnan : (q < 2 * nm ? it.predicted_px[q] : 0.0);
    wins[4 * k] = it.roi_h;
    wins[4 * k + 1] = it.roi_w;
    wins[4 * k + 2] = it.roi_x;
    wins[4 * k + 3] = it.roi_y;
    gat[k] = GatherItem{it.img, it.roi_x, it.roi_y, it.roi_w, it.roi_h, k, 0};
  }
  uint8_t* host_rec = mb + ((head_bytes + 255) & ~(size_t)255);
  if ((rc = reserve_track(h, g, n, in_bytes)) != MPE_OK) return rc;
  uint8_t* d_in = static_cast<uint8_t*>(h->frames.p);
  h->have_ms = false;
  if (h->track_profile) pt.t_packed = clk::now();
  HIP_TRY(h, hipMemcpyAsync(d_in, mb, head_bytes, hipMemcpyHostToDevice, h->stream));
  pt.g = g;
  pt.slot_bytes = slot;
  pt.rec_bytes = rec_bytes;
  pt.d_pred = reinterpret_cast<const double*>(d_in);
  pt.d_wins = d_in + pred_bytes;
  pt.d_pix = d_in + head_bytes;
  HIP_TRY(h, launch_gather_rois(reinterpret_cast<const GatherItem*>(d_in + gat_off), n, d_in + head_bytes, g, stride_bytes,
                                img_bytes, h->stream));
  ++h->track_batch_submits;
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
}  // namespace

extern "C" {

int mpe_track_step_batch_setups_device_submit(mpe_handle* h, const mpe_track_item* items, const int* item_setup, int n,
                                              int rows, int cols, size_t stride_bytes, const mpe_track_setup* setups,
                                              int n_setups) {
  // every usage error before any device work, with the codes and messages of mpe_track_step_batch_setups_submit
  if (!h || !items || n < 0 || !setups || n_setups < 1 || (!item_setup && n_setups != 1) || rows < 1 || cols < 1 ||
      stride_bytes < (size_t)cols)
    return fail(h, MPE_ERR_ARG, "bad argument");
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
    if (!items[i].img || !roi_inside(items[i], rows, cols)) return fail(h, MPE_ERR_ARG, "ROI outside the image");
    used[(size_t)s] = 1;
    rmax = std::max(rmax, items[i].roi_h);
    wmax = std::max(wmax, items[i].roi_w);
  }
  if (n == 0) return MPE_OK;
  FrameGeom g;
  if (make_geom(h, rmax, wmax, g)) return fail(h, MPE_ERR_UNSUPPORTED, "frame size unsupported");
  std::vector<TrackSetup> prep((size_t)n_setups);
  for (int s = 0; s < n_setups; ++s) {  // (the set-ups that have streams)
    const mpe_track_setup& su = setups[s];
    if (!used[(size_t)s]) continue;
    if (make_detect_params(su.p, su.K, su.D, su.nD, 0, 0, prep[(size_t)s].dp)) return fail(h, MPE_ERR_ARG, "gaussian_sigma must be in (0, 6]");
    if (make_solve_params(h, su.p, su.markers_xyz, su.n_markers, su.K, prep[(size_t)s].sp)) return fail(h, MPE_ERR_ARG, "bad set-up");
    prep[(size_t)s].nn_tol = su.p->nearest_neighbour_pixel_tolerance;
  }
  ENTER(h);
  const size_t img_bytes = (size_t)(rows - 1) * stride_bytes + (size_t)cols;
  const int rc = check_device_images(h, items, n, img_bytes);
  if (rc != MPE_OK) return rc;
  return submit_device_slots(h, items, item_setup, n, g, stride_bytes, img_bytes, prep.data(), n_setups);
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

}  // extern "C"
