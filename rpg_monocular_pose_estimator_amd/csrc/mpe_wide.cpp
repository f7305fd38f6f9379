// mpe_wide.cpp — host side of libmpe_hip.so, part 5 (see mpe_host.h): the *_wide entries of include/mpe.h — detection sets
// of up to MPE_WIDE_DETECTIONS points (a frame on which more than MPE_MAX_DETECTIONS blobs pass the shape filter), a
// surface of its own beside the ordinary entries, which keep their records, capacities and answers.
#include "mpe_host.h"

namespace {
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// a table beyond this many blocks (hundreds of full sets in one call) is built with fewer blocks per set
constexpr size_t kWideMaxBlocks = (size_t)1 << 18;

// every usage error of the two entries, before any device work
int wide_usage(mpe_handle* h, const double* det_xy, const int* n_det, int n, const double* markers_xyz, int n_markers,
               const double* K) {
  if (!h || !det_xy || !n_det || n < 0 || !markers_xyz || !K) return fail(h, MPE_ERR_ARG, "bad argument");
  if (n_markers < 1 || n_markers > MPE_MAX_MARKERS) return fail(h, MPE_ERR_ARG, "n_markers outside 1 .. MPE_MAX_MARKERS");
  for (int i = 0; i < n; ++i)
    if (n_det[i] < 0 || n_det[i] > MPE_WIDE_DETECTIONS) return fail(h, MPE_ERR_ARG, "n_det outside 0 .. MPE_WIDE_DETECTIONS");
  if (n > 0 && (h->pending_track_n || h->submit_seq != h->collect_seq))
    return fail(h, MPE_ERR_ARG, "a submitted batch has not been collected yet");
  return MPE_OK;
}

// The block table of n sets of one marker set (mpe_brute_blocks.h): one block per 1024 hypotheses, at most four blocks
// per compute unit for one set (option "wide_block_cap" overrides), fewer when the table would pass kWideMaxBlocks.
void wide_block_table(const mpe_handle* h, const int* n_det, int n, int n_markers, std::vector<BruteBlock>& blocks) {
  int cap = h->wide_block_cap > 0 ? h->wide_block_cap : 4 * std::max(1, device_cu_count());
  const std::vector<int> nm((size_t)n, n_markers);
  for (;;) {
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += (size_t)brute_parts(brute_hypotheses(n_det[i], n_markers), cap);
    if (total <= kWideMaxBlocks || cap <= 1) break;
    cap = std::max(1, cap / 2);
  }
  brute_block_table(n_det, nm.data(), n, cap, blocks);
}

// [wide detection records | block table] into the pinned staging memory; returns the table's offset
size_t wide_stage_input(uint8_t* mb, const double* det_xy, const int* n_det, int n, const std::vector<BruteBlock>& blocks) {
  const size_t blk_off = up256((size_t)n * sizeof(mpe_detections_wide));
  mpe_detections_wide* hd = reinterpret_cast<mpe_detections_wide*>(mb);
  std::memset(mb, 0, blk_off);
  for (int f = 0; f < n; ++f) {
    hd[f].n = n_det[f];
    std::memcpy(hd[f].undist_xy, det_xy + (size_t)f * 2 * MPE_WIDE_DETECTIONS, sizeof(double) * 2 * n_det[f]);
  }
  if (!blocks.empty()) std::memcpy(mb + blk_off, blocks.data(), blocks.size() * sizeof(BruteBlock));
  return blk_off;
}
}  // namespace

extern "C" {

int mpe_vote_batch_wide(mpe_handle* h, const double* det_xy, const int* n_det, int n_frames, const double* markers_xyz,
                        int n_markers, const double K[9], double back_projection_pixel_tolerance, uint32_t* hist) {
  { const int rc = wide_usage(h, det_xy, n_det, n_frames, markers_xyz, n_markers, K); if (rc != MPE_OK) return rc; }
  if (!hist) return fail(h, MPE_ERR_ARG, "bad argument");
  if (n_frames == 0) return MPE_OK;
  if (h->vote_arith == 2) return fail(h, MPE_ERR_UNSUPPORTED, "vote_arith 2 has no strict form: the wide entries vote with the strict arithmetic");
  ENTER(h);
  mpe_params p;
  mpe_default_params(&p);
  p.back_projection_pixel_tolerance = back_projection_pixel_tolerance;
  SolveParams sp;
  if (make_solve_params(h, &p, markers_xyz, n_markers, K, sp)) return fail(h, MPE_ERR_ARG, "too many markers");
  std::vector<BruteBlock> blocks;
  wide_block_table(h, n_det, n_frames, n_markers, blocks);
  const size_t head_bytes = up256((size_t)n_frames * sizeof(mpe_detections_wide)) + blocks.size() * sizeof(BruteBlock);
  const size_t hist_bytes = (size_t)n_frames * MPE_WIDE_HIST_STRIDE * sizeof(uint32_t);
  { const int rc = grow_mailbox(h, head_bytes); if (rc != MPE_OK) return rc; }
  uint8_t* mb = static_cast<uint8_t*>(h->mailbox);
  const size_t blk_off = wide_stage_input(mb, det_xy, n_det, n_frames, blocks);
  HIP_TRY(h, h->frames.reserve(head_bytes));
  HIP_TRY(h, h->hist.reserve(hist_bytes));
  uint8_t* d_in = static_cast<uint8_t*>(h->frames.p);
  uint32_t* d_hist = static_cast<uint32_t*>(h->hist.p);
  HIP_TRY(h, hipMemcpyAsync(d_in, mb, head_bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemsetAsync(d_hist, 0, hist_bytes, h->stream));
  HIP_TRY(h, launch_k2_vote_wide(reinterpret_cast<const mpe_detections_wide*>(d_in), sp,
                                 reinterpret_cast<const BruteBlock*>(d_in + blk_off), (int)blocks.size(), d_hist, h->stream));
  HIP_TRY(h, hipMemcpy2DAsync(hist, MPE_WIDE_HIST_WORDS * sizeof(uint32_t), d_hist, MPE_WIDE_HIST_STRIDE * sizeof(uint32_t),
                              MPE_WIDE_HIST_WORDS * sizeof(uint32_t), (size_t)n_frames, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return MPE_OK;
}

int mpe_solve_bruteforce_batch_wide(mpe_handle* h, const double* det_xy, const int* n_det, int n,
                                    const double* markers_xyz, int n_markers, const double K[9], const mpe_params* p,
                                    mpe_result* out, uint32_t* hist, uint32_t* corr) {
  { const int rc = wide_usage(h, det_xy, n_det, n, markers_xyz, n_markers, K); if (rc != MPE_OK) return rc; }
  if (!p || !out) return fail(h, MPE_ERR_ARG, "bad argument");
  if (n == 0) return MPE_OK;
  if (h->vote_arith == 2) return fail(h, MPE_ERR_UNSUPPORTED, "vote_arith 2 has no strict form: the wide entries vote with the strict arithmetic");
  ENTER(h);
  SolveParams sp;
  if (make_solve_params(h, p, markers_xyz, n_markers, K, sp)) return fail(h, MPE_ERR_ARG, "too many markers");
  std::vector<BruteBlock> blocks;
  wide_block_table(h, n_det, n, n_markers, blocks);
  // in: [wide records | block table]; back: [records | correspondence rows (compact indices) | slot -> wide index |
  // histograms]; on the device alone: the compact records and the rows handed to the validation kernel
  const size_t head_bytes = up256((size_t)n * sizeof(mpe_detections_wide)) + blocks.size() * sizeof(BruteBlock);
  const size_t res_bytes = (size_t)n * sizeof(mpe_result), corr_bytes = (size_t)n * 2 * MPE_MAX_MARKERS * sizeof(uint32_t);
  const size_t slot_bytes = (size_t)n * MPE_MAX_MARKERS * sizeof(uint32_t);
  const size_t hist_off = up256(res_bytes + corr_bytes + slot_bytes);
  const size_t hist_bytes = (size_t)n * MPE_WIDE_HIST_STRIDE * sizeof(uint32_t);
  const size_t back_bytes = hist ? hist_off + hist_bytes : res_bytes + corr_bytes + slot_bytes;
  const size_t back_off = up256(head_bytes);
  { const int rc = grow_mailbox(h, back_off + back_bytes); if (rc != MPE_OK) return rc; }
  uint8_t* mb = static_cast<uint8_t*>(h->mailbox);
  const size_t blk_off = wide_stage_input(mb, det_xy, n_det, n, blocks);
  HIP_TRY(h, h->frames.reserve(head_bytes));
  HIP_TRY(h, h->results.reserve(hist_off + hist_bytes));
  HIP_TRY(h, h->dets.reserve((size_t)n * sizeof(mpe_detections)));
  HIP_TRY(h, h->corr.reserve(corr_bytes));
  HIP_TRY(h, h->mid.reserve(k3_mid_bytes(n)));
  uint8_t* d_in = static_cast<uint8_t*>(h->frames.p);
  uint8_t* d_back = static_cast<uint8_t*>(h->results.p);
  const mpe_detections_wide* d_wide = reinterpret_cast<const mpe_detections_wide*>(d_in);
  mpe_result* d_res = reinterpret_cast<mpe_result*>(d_back);
  uint32_t* d_corr = reinterpret_cast<uint32_t*>(d_back + res_bytes);
  uint32_t* d_slot = reinterpret_cast<uint32_t*>(d_back + res_bytes + corr_bytes);
  uint32_t* d_hist = reinterpret_cast<uint32_t*>(d_back + hist_off);
  mpe_detections* d_compact = static_cast<mpe_detections*>(h->dets.p);
  uint32_t* d_rows = static_cast<uint32_t*>(h->corr.p);
  ++h->bruteforce_submits;
  HIP_TRY(h, hipMemcpyAsync(d_in, mb, head_bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemsetAsync(d_hist, 0, hist_bytes, h->stream));
  HIP_TRY(h, launch_k2_vote_wide(d_wide, sp, reinterpret_cast<const BruteBlock*>(d_in + blk_off), (int)blocks.size(), d_hist,
                                 h->stream));
  HIP_TRY(h, launch_k3_peel_wide(d_wide, d_hist, n, sp.n_markers, sp.hist_thr, d_compact, d_rows, d_slot, h->stream));
  // (the validation kernel takes its rows from d_rows and never reads a histogram: the pointer is only offset)
  HIP_TRY(h, launch_k3_tail(d_compact, d_hist, n, sp, d_res, d_corr, d_rows, nullptr, 0.0, h->mid.p, h->stream, 0));
  HIP_TRY(h, hipMemcpyAsync(mb + back_off, d_back, back_bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < n; ++i) h->wide_frames += n_det[i] > MPE_MAX_DETECTIONS ? 1 : 0;
  // hand out: the rows back in the caller's indices, n_det the caller's count
  const mpe_result* b_res = reinterpret_cast<const mpe_result*>(mb + back_off);
  const uint32_t* b_corr = reinterpret_cast<const uint32_t*>(mb + back_off + res_bytes);
  const uint32_t* b_slot = reinterpret_cast<const uint32_t*>(mb + back_off + res_bytes + corr_bytes);
  for (int i = 0; i < n; ++i) {
    out[i] = b_res[i];
    out[i].n_det = n_det[i];
    if (!corr) continue;
    uint32_t* co = corr + (size_t)i * 2 * MPE_MAX_MARKERS;
    std::memset(co, 0, 2 * MPE_MAX_MARKERS * sizeof(uint32_t));
    for (int r = 0; r < out[i].n_corr && r < MPE_MAX_MARKERS; ++r) {
      const uint32_t m = b_corr[(size_t)i * 2 * MPE_MAX_MARKERS + 2 * r], s = b_corr[(size_t)i * 2 * MPE_MAX_MARKERS + 2 * r + 1];
      co[2 * r] = m;
      co[2 * r + 1] = (s >= 1 && s <= MPE_MAX_MARKERS) ? b_slot[(size_t)i * MPE_MAX_MARKERS + (s - 1)] : 0u;
    }
  }
  if (hist)  // (device rows are MPE_WIDE_HIST_STRIDE words apart, the caller's MPE_WIDE_HIST_WORDS)
    for (int f = 0; f < n; ++f)
      std::memcpy(hist + (size_t)f * MPE_WIDE_HIST_WORDS,
                  mb + back_off + hist_off + (size_t)f * MPE_WIDE_HIST_STRIDE * sizeof(uint32_t),
                  MPE_WIDE_HIST_WORDS * sizeof(uint32_t));
  return MPE_OK;
}

int mpe_detect_batch_wide(mpe_handle* h, const uint8_t* frames, int n_frames, int rows, int cols, size_t stride_bytes,
                          size_t frame_stride_bytes, int frames_on_device, const double K[9], const double* D, int nD,
                          const mpe_params* p, mpe_detections_wide* dets) {
  if (!h || !frames || !p || !K || !dets || n_frames < 0) return fail(h, MPE_ERR_ARG, "bad argument");
  if (n_frames == 0) return MPE_OK;
  if (h->pending_track_n || h->submit_seq != h->collect_seq)
    return fail(h, MPE_ERR_ARG, "a submitted batch has not been collected yet");
  ENTER(h);
  FrameGeom g;
  if (make_geom(h, rows, cols, g)) return fail(h, MPE_ERR_UNSUPPORTED, "frame size unsupported");
  DetectParams dp;
  if (make_detect_params(p, K, D, nD, 0, 0, dp)) return fail(h, MPE_ERR_ARG, "gaussian_sigma must be in (0, 6]");
  const uint8_t* d_frames = nullptr;
  { const int rc = stage_frames(h, frames, n_frames, rows, cols, stride_bytes, frame_stride_bytes, frames_on_device, 0, 0,
                                cols, rows, g, &d_frames); if (rc) return rc; }
  // scan, then the general tier over ALL frames of the call (work-list: the identity), with the wide writer
  const size_t bytes = (size_t)n_frames * g.rows * g.pitch;
  HIP_TRY(h, h->flags.reserve(flag_words(bytes) * 8));
  HIP_TRY(h, h->work.reserve((size_t)(n_frames + 1) * sizeof(int)));
  HIP_TRY(h, h->scratch.reserve(k1b_scratch_bytes(g, n_frames)));
  HIP_TRY(h, h->results.reserve((size_t)n_frames * sizeof(mpe_detections_wide)));
  std::vector<int> list((size_t)n_frames + 1);
  list[0] = n_frames;
  for (int f = 0; f < n_frames; ++f) list[(size_t)f + 1] = f;
  unsigned long long* d_flags = static_cast<unsigned long long*>(h->flags.p);
  mpe_detections_wide* d_dets = static_cast<mpe_detections_wide*>(h->results.p);
  HIP_TRY(h, hipMemcpyAsync(h->work.p, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (list goes out of scope; pageable memory)
  HIP_TRY(h, launch_k1a_scan(d_frames, bytes, d_flags, dp.thr, 0, h->stream));
  HIP_TRY(h, launch_k1b_general_wide(d_frames, d_flags, n_frames, g, dp, d_dets, static_cast<const int*>(h->work.p),
                                     static_cast<uint8_t*>(h->scratch.p), h->scratch.cap, h->stream, h->general_lds == 1));
  HIP_TRY(h, hipMemcpyAsync(dets, d_dets, (size_t)n_frames * sizeof(mpe_detections_wide), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return MPE_OK;
}

int mpe_estimate_batch_wide(mpe_handle* h, const uint8_t* frames, int n_frames, int rows, int cols, size_t stride_bytes,
                            size_t frame_stride_bytes, int frames_on_device, const double* markers_xyz, int n_markers,
                            const double K[9], const double* D, int nD, const mpe_params* p, mpe_result* results) {
  if (!h || !frames || !markers_xyz || !K || !p || !results || n_frames < 0) return fail(h, MPE_ERR_ARG, "bad argument");
  if (n_markers < 1 || n_markers > MPE_MAX_MARKERS) return fail(h, MPE_ERR_ARG, "n_markers outside 1 .. MPE_MAX_MARKERS");
  if (n_frames == 0) return MPE_OK;
  if (h->pending_track_n || h->submit_seq != h->collect_seq)
    return fail(h, MPE_ERR_ARG, "a submitted batch has not been collected yet");
  int rc = mpe_estimate_batch(h, frames, n_frames, rows, cols, stride_bytes, frame_stride_bytes, frames_on_device,
                              markers_xyz, n_markers, K, D, nD, p, results);
  if (rc != MPE_OK) return rc;
  // the frames whose record says "more than MPE_MAX_DETECTIONS blobs passed": detection again with the wide record (a
  // call per frame: such frames are rare), then ONE wide solve over those that fit it
  std::vector<int> wide;
  for (int f = 0; f < n_frames; ++f)
    if (results[f].status == MPE_FRAME_TOO_MANY_DETECTIONS) wide.push_back(f);
  if (wide.empty()) return MPE_OK;
  // (only now: a batch without such a frame is mpe_estimate_batch under every vote_arith)
  if (h->vote_arith == 2) return fail(h, MPE_ERR_UNSUPPORTED, "vote_arith 2 has no strict form: the wide entries vote with the strict arithmetic");
  std::vector<double> xy;
  std::vector<int> nd, idx;
  mpe_detections_wide dw;
  for (int f : wide) {
    rc = mpe_detect_batch_wide(h, frames + (size_t)f * frame_stride_bytes, 1, rows, cols, stride_bytes, frame_stride_bytes,
                               frames_on_device, K, D, nD, p, &dw);
    if (rc != MPE_OK) return rc;
    if (dw.status != 0) {  // (more than MPE_WIDE_DETECTIONS blobs, or a band capacity: the code stays, never silent)
      results[f].status = dw.status;
      results[f].n_det = dw.n;
      continue;
    }
    idx.push_back(f);
    nd.push_back(dw.n);
    xy.resize(xy.size() + (size_t)2 * MPE_WIDE_DETECTIONS, 0.0);
    std::memcpy(&xy[xy.size() - (size_t)2 * MPE_WIDE_DETECTIONS], dw.undist_xy, sizeof(double) * 2 * dw.n);
  }
  if (idx.empty()) return MPE_OK;
  std::vector<mpe_result> out(idx.size());
  const long long before = h->wide_frames;
  rc = mpe_solve_bruteforce_batch_wide(h, xy.data(), nd.data(), (int)idx.size(), markers_xyz, n_markers, K, p, out.data(),
                                       nullptr, nullptr);
  if (rc != MPE_OK) return rc;
  h->wide_frames = before + (long long)idx.size();  // (every frame solved here counts, whatever the wide detection found)
  for (size_t k = 0; k < idx.size(); ++k) results[idx[k]] = out[k];
  return MPE_OK;
}

}  // extern "C"
