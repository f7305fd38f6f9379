"""Detection and tracking at the frame-size capacity: make_geom (csrc/mpe_schedule.cpp) takes frames of up to 4096 rows
(s_rowact[64]: a bit per row) by 4000 columns (a bitmap row of at most 64 words), and the blob kernels have bitsets,
packed keys and branches that only such frames reach — the row bitset's words 19 .. 63, s_colocc words 2 and 3, a whole
wave per bitmap row (lw = 6, from 1983 columns on; at 4000 columns lane == word with no lane to spare), the whole-frame
scan of a frame with more than 768 bands, y << 12 | x keys with y up to 4095 and x up to 3999, ROI origins beyond
(2048, 1200) in the repack, gather and decode kernels.  The frames come from tests/frame_size_cases.py: ten narrow shapes,
each the smallest that reaches the structure it is named for, and the full 4096 x 4000 frame in three tests, two frames
each.  The reference is the CPU oracle, to the bit for detections and within POS_TOL_M / ROT_TOL_RAD for poses; on the
narrow shapes the oracle itself is held to the numpy witness (tests/witness_pipeline.py) by the CPU test at the top.
What ran is asserted from numbers that do not come out of the kernels: wb and lw from the frame size by make_geom's
formula, the band count the band frames guarantee by how they were drawn, and the "general_seen" read-out (it follows
batches of 64 frames or more, so it is asserted on the narrow shapes; at full size that would be 1 GB of frames).
Met on the way and fixed: make_geom refused every frame and ROI of 1 .. 3 rows (the one-row ROI on the last row of the
full-size frame); test_frames_and_windows_of_one_to_three_rows holds the other end of the size range since.
(The CPU tier runs the same frames through the host build of the device source: tests/test_k1b_host.py.)

Measured: the oracle's find_leds takes 0.18 - 0.25 s on a 4096 x 4000 frame (0.5 s of oracle time in each of the three
full-size tests, 0.9 s to draw the two frames), 2 ms on a narrow shape.  The GPU tier of this file takes 26 s on an
MI355X (24 tests; the slowest, 4.5 s each, are the 4096- and 4095-row shapes, whose batches of 64 frames — what the
"general_seen" read-out needs — go through the general tier twice); the two CPU tests at the top 1.6 s."""
import numpy as np
import pytest

import rpg_monocular_pose_estimator_amd as mpe
from rpg_monocular_pose_estimator_amd import synth
import frame_size_cases as fsc
from util import pose_diff, POS_TOL_M, ROT_TOL_RAD

MPE_ERR_ARG, MPE_ERR_UNSUPPORTED = -1, -3
ROWS, COLS = fsc.FULL
BAND_CASES = [(4096, 33, fsc.BAND_SIGMA, 6), (4095, 33, fsc.BAND_SIGMA, 6), (1537, 33, fsc.TIGHT_SIGMA, 0),
              (1600, 48, fsc.TIGHT_SIGMA, 2), (1536, 33, fsc.TIGHT_SIGMA, 0)]
_REF = {}


def _ref(orc, key, img, K, D, roi=None, **kw):
    """The oracle's (undist, dist) of one frame, computed once."""
    key = (key, roi, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = orc.find_leds(img, orc.make_params(**kw), K, D, roi=roi)
    return _REF[key]


def _same_detections(rec, und, dist, what):
    """One detection record of the library against the oracle's lists: count, order, bytes."""
    n = len(und)
    assert rec["status"] == 0 and rec["n"] == n, (what, int(rec["status"]), int(rec["n"]), n)
    assert rec["dist_xy"][:2 * n].tobytes() == np.ascontiguousarray(dist, np.float32).tobytes(), what
    assert rec["undist_xy"][:2 * n].tobytes() == np.ascontiguousarray(und, np.float64).tobytes(), what


def _canon(recs):
    """What a batch of detection records says: (n, status, the first n points) of each — the bytes behind them are not
    written and say nothing."""
    return [(int(r["n"]), int(r["status"]), r["undist_xy"][:2 * max(int(r["n"]), 0)].tobytes(),
             r["dist_xy"][:2 * max(int(r["n"]), 0)].tobytes()) for r in recs]


def _far_roi(rows, cols):
    """The far quarter less a row and a column: an odd origin beyond the middle, touching the last row and column."""
    return (cols // 2 + 1, rows // 2 + 1, cols - cols // 2 - 1, rows - rows // 2 - 1)


def _detect_everywhere(hip, orc, name, img, K, D, rois, expect_general, **kw):
    """detect_batch, detect_batch_wide and find_leds (whole image and ROIs) under both kernels of the general tier: the
    oracle's records, and identical records in both settings (a shape whose bitmaps do not fit k1b_general_lds falls
    back by itself).  expect_general: the frame must reach the general tier — shown by the read-out "general_seen" after
    a batch of 64 copies of it, whose records are those of the single frame."""
    Ph = mpe.demo_params(**kw)
    und, dist = _ref(orc, name, img, K, D, **kw)
    assert len(und) <= mpe.MAX_DETECTIONS
    got = {}
    try:
        for lds in (0, 1):
            hip.set_option("general_lds", lds)
            rec = hip.detect_batch(img[None], K, D, Ph)
            _same_detections(rec[0], und, dist, (name, lds, "detect_batch"))
            if expect_general:      # (the read-out follows batches of 64 frames or more: run_front, csrc/mpe_schedule.cpp)
                many = hip.detect_batch(np.ascontiguousarray(np.broadcast_to(img, (64,) + img.shape)), K, D, Ph)
                seen = hip.get_option("general_seen")
                assert seen == 64, (name, lds, seen)
                assert _canon(many) == _canon(rec) * 64, (name, lds)
            wide = hip.detect_batch_wide(img[None], K, D, Ph)
            _same_detections(wide[0], und, dist, (name, lds, "detect_batch_wide"))
            got[lds] = [_canon(rec), _canon(wide)]
            for roi in [None] + list(rois):
                uo, do = _ref(orc, name, img, K, D, roi=roi, **kw)
                uh, dh = hip.find_leds(img, Ph, K, D, roi=roi)
                assert dh.tobytes() == do.tobytes() and uh.tobytes() == uo.tobytes(), (name, lds, roi, len(dh), len(do))
                got[lds].append(uh.tobytes())
    finally:
        hip.set_option("general_lds", 0)
    assert got[0] == got[1], name
    return len(und)


# ---- CPU tier ----------------------------------------------------------------------------------------------------------

def test_oracle_equals_the_witness_on_the_narrow_shapes(orc):
    """The oracle is pinned by golden vectors up to 1920 x 1200 only; on the narrow capacity shapes, plain and salted,
    it gives the bytes of the numpy witness (scipy components + Moore tracing)."""
    import witness_pipeline as W
    n = 0
    for rows, cols in fsc.NARROW:
        K, D = synth.camera_for(rows, cols)
        for clutter in (False, True):
            img = fsc.frame(rows, cols, clutter)["img"]
            und, dist = _ref(orc, (rows, cols, clutter), img, K, D)
            wu, wd = W.find_leds(img, 140, 0.6, 10.0, 200.0, 0.5, 0.5, K, D)
            assert wd.tobytes() == dist.tobytes() and wu.tobytes() == und.tobytes(), (rows, cols, clutter)
            n += len(und)
    assert n >= 100, n


def test_far_quarter_scene_is_posed_by_the_oracle(orc):
    """The precondition of the end-to-end checks: all five LEDs of both frames lie in x >= 2000, y >= 2048 and the oracle
    has a pose on both."""
    s = _scene(orc)
    assert s["px"][..., 0].min() >= COLS / 2 and s["px"][..., 1].min() >= ROWS / 2
    assert (s["ref"]["status"] == 0).all() and (s["ref"]["n_det"] == 5).all(), (s["ref"]["status"], s["ref"]["n_det"])


def _scene(orc):
    if "scene" not in _REF:
        s = fsc.far_quarter_scene(2)
        s["ref"] = orc.estimate_batch(s["frames"], s["markers"], s["K"], s["D"], orc.make_params(), n_threads=2)
        _REF["scene"] = s
    return _REF["scene"]


def _oracle_track(orc, img, roi, K, D, markers, pred, nn_tol):
    """findLeds(ROI) + findCorrespondences + checkCorrespondences + optimisePose from the oracle's pieces (as
    test_gpu_parity.test_track_step_matches_oracle_pieces assembles them) -> (und, corr, ok, T)."""
    Po = orc.make_params()
    und, _ = orc.find_leds(img, Po, K, D, roi=roi)
    corr = []
    if len(und) >= 4:
        for m in range(len(pred)):
            dist = np.sqrt(((und - pred[m]) ** 2).sum(axis=1))
            j = int(np.argmin(dist))
            if dist[j] <= nn_tol:
                corr.append((m + 1, j + 1))
    corr = np.array(corr, np.uint32).reshape(-1, 2)
    ok, T0 = orc.check_correspondences(und, markers, K, Po, corr) if len(corr) >= 4 else (False, None)
    T = orc.optimise_pose(und, markers, K, corr, T0)[0] if ok else None
    return und, corr, bool(ok), T


# ---- GPU tier: detection -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", fsc.NARROW, ids=["%dx%d" % s for s in fsc.NARROW])
def test_detection_on_the_narrow_shapes(hip, orc, rows, cols):
    """Every detection entry on one narrow shape, plain and with the far-quarter salt (the general tier, by the
    "general_seen" read-out), whole image, ROIs in the far quarter and on the last 1 .. 3 rows and the last column."""
    g = fsc.geom(rows, cols)
    want = {(17, 4000): (64, 6), (17, 3999): (64, 6), (17, 3967): (64, 6), (17, 3966): (63, 6), (17, 1983): (33, 6),
            (17, 1982): (32, 5)}.get((rows, cols))
    assert want is None or (g["wb"], g["lw"]) == want
    assert rows < 4095 or g["rw"] == 64
    K, D = synth.camera_for(rows, cols)
    # (the last rows alone, 1 .. 3 of them: whether the LDS budget holds a width does not depend on the frame's height)
    rois = [_far_roi(rows, cols), (cols - 9, 0, 9, rows), (0, rows - 9, cols, 9), (0, rows - 1, cols, 1),
            (cols // 2, rows - 2, cols - cols // 2, 2), (1, rows - 3, cols - 1, 3), (cols - 1, 0, 1, rows)]
    for clutter in (False, True):
        n = _detect_everywhere(hip, orc, (rows, cols, clutter), fsc.frame(rows, cols, clutter)["img"], K, D, rois, clutter)
        assert n >= 6, (rows, cols, n)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,sigma,n_spots", BAND_CASES, ids=["%dx%d-sigma%.1f" % c[:3] for c in BAND_CASES])
def test_detection_with_more_bands_than_the_band_list(hip, orc, rows, cols, sigma, n_spots):
    """The band frames: more than 768 bands — by how the frame was drawn — on every shape but the 1536-row control
    (exactly 768: the last frame the band list holds), in the general tier; the lone pixels are dropped, the spots kept."""
    b = fsc.band_frame(rows, cols, sigma, n_spots)
    assert (b["n_bands"] > fsc.GEN_BANDS) == (rows != 1536), (rows, b["n_bands"])
    assert rows != 1536 or b["n_bands"] == fsc.GEN_BANDS
    K, D = synth.camera_for(rows, cols)
    n = _detect_everywhere(hip, orc, ("band", rows, cols, sigma), b["img"], K, D, [_far_roi(rows, cols)], True, gaussian_sigma=sigma)
    assert n == n_spots, (rows, cols, n)


@pytest.mark.gpu
def test_detection_and_rois_on_the_full_size_frame(hip, orc):
    """4096 x 4000, two frames in one batch (the plain one and, at frame index 1 — 16.4 MB into the batch — the salted
    one): detect_batch and detect_batch_wide under both general-tier kernels, then find_leds through ROIs whose origin
    lies beyond (2048, 1200) — as given, and as determine_roi clips them from predictions at the corner."""
    g = fsc.geom(ROWS, COLS)
    assert (g["wb"], g["lw"], g["rw"], g["pitch"]) == (64, 6, 64, COLS)
    K, D = synth.camera_for(ROWS, COLS)
    frames = np.stack([fsc.frame(ROWS, COLS)["img"], fsc.frame(ROWS, COLS, True)["img"]])
    refs = [_ref(orc, (ROWS, COLS, c), frames[c], K, D) for c in (0, 1)]
    assert 15 <= len(refs[0][0]) <= mpe.MAX_DETECTIONS and refs[1][1].tobytes() == refs[0][1].tobytes()
    # (no "general_seen" here: the read-out follows batches of 64 frames or more, 1 GB at this size.  The salted frame has
    #  a bright segment per salt pixel, far more than the 512 the larger LDS tier lists: it cannot stay there.)
    assert fsc.frame(ROWS, COLS, True)["n_salt"] > 50000
    Ph = mpe.demo_params()
    got = {}
    try:
        for lds in (0, 1):
            hip.set_option("general_lds", lds)
            rec = hip.detect_batch(frames, K, D, Ph)
            wide = hip.detect_batch_wide(frames, K, D, Ph)
            for i in (0, 1):
                _same_detections(rec[i], *refs[i], (lds, i))
                _same_detections(wide[i], *refs[i], (lds, i, "wide"))
            got[lds] = _canon(rec) + _canon(wide)
    finally:
        hip.set_option("general_lds", 0)
    assert got[0] == got[1]
    # predictions are undistorted pixels: those of the spots the oracle found at the corner and on x = 2047/2048 of the
    # lower rows lie far outside the image (k1 < 0), and determine_roi brings their box back in and clips it
    und, dist = refs[1]
    corner = und[(dist[:, 0] > COLS - 60) & (dist[:, 1] > ROWS - 60)]
    inner = und[(np.abs(dist[:, 0] - 2024) < 30) & (np.abs(dist[:, 1] - 4031.5) < 4)]
    assert len(corner) == 1 and len(inner) == 2 and corner.max() > ROWS + 100
    clipped = [orc.determine_roi(p, ROWS, COLS, 20, K, D) for p in (corner, inner)]
    assert clipped == [mpe.determine_roi(p, ROWS, COLS, 20, K, D) for p in (corner, inner)]
    assert clipped[0][0] + clipped[0][2] >= COLS - 1 and clipped[0][1] + clipped[0][3] >= ROWS - 1 and clipped[0][2] < 40  # cut by both edges
    n = 0
    for roi in fsc.FULL_ROIS + clipped + [_far_roi(ROWS, COLS)]:
        assert roi[0] >= 1980 and roi[1] >= 2048, roi
        uo, do = orc.find_leds(frames[1], orc.make_params(), K, D, roi=roi)
        uh, dh = hip.find_leds(frames[1], Ph, K, D, roi=roi)
        assert dh.tobytes() == do.tobytes() and uh.tobytes() == uo.tobytes(), (roi, len(dh), len(do))
        n += len(do)
    assert n >= 6, n


# ---- GPU tier: end to end ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_estimate_batch_in_the_far_quarter_of_a_full_size_frame(hip, orc):
    """The C2 markers projected into x >= 2000, y >= 2048 of two 4096 x 4000 frames: mpe_estimate_batch (host frames) and
    mpe_estimate_batch_device, with "pipeline" 1 and 16 — status, n_det, n_corr the oracle's, poses within POS_TOL_M /
    ROT_TOL_RAD."""
    import torch
    s = _scene(orc)
    ro = s["ref"]
    assert (ro["status"] == 0).all()
    d_frames = torch.from_numpy(s["frames"]).cuda()
    before = hip.get_option("pipeline")
    try:
        for pipeline in (1, 16):
            hip.set_option("pipeline", pipeline)
            res = torch.zeros(2 * mpe.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=d_frames.device)
            hip.estimate_batch_device(d_frames.data_ptr(), 2, ROWS, COLS, s["markers"], s["K"], s["D"], mpe.demo_params(),
                                      res.data_ptr())
            hip.synchronize()
            torch.cuda.synchronize()
            dev = np.frombuffer(res.cpu().numpy().tobytes(), mpe.RESULT_DTYPE)
            host = hip.estimate_batch(s["frames"], s["markers"], s["K"], s["D"], mpe.demo_params())
            for what, rh in (("host", host), ("device", dev)):
                assert np.array_equal(rh["status"], ro["status"]) and np.array_equal(rh["n_det"], ro["n_det"]), (what, pipeline)
                assert np.array_equal(rh["n_corr"], ro["n_corr"]), (what, pipeline)
                for i in range(2):
                    dp, dr = pose_diff(rh["T"][i], ro["T"][i])
                    assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (what, pipeline, i, dp, dr)
    finally:
        hip.set_option("pipeline", before)


# ---- GPU tier: the tracked path ------------------------------------------------------------------------------------------

def _check_item(orc, det, corr, res, img, roi, K, D, markers, pred, what):
    """One item of a tracked call against the oracle's chain: undist to the bit, correspondences equal, pose within the
    tolerances.  -> whether the oracle has a pose."""
    nn_tol = mpe.demo_params().nearest_neighbour_pixel_tolerance
    und, _ = orc.find_leds(img, orc.make_params(), K, D, roi=roi)
    n = len(und)
    assert det["status"] == 0 and det["n"] == n, (what, int(det["status"]), int(det["n"]), n)
    assert det["undist_xy"][:2 * n].tobytes() == und.tobytes(), what
    if pred is None:
        return False
    _, co, ok, T = _oracle_track(orc, img, roi, K, D, markers, pred, nn_tol)
    assert (res["status"] == 0) == ok and np.array_equal(corr[:max(int(res["n_corr"]), 0)], co), (what, int(res["status"]), ok)
    if ok:
        dp, dr = pose_diff(res["T"], T)
        assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (what, dp, dr)
    return ok


@pytest.mark.gpu
def test_tracked_frames_at_full_size(hip, orc):
    """mpe_track_step with a ROI in the far corner of a 4096 x 4000 frame, then ONE lock-step call of three streams of
    4096 x 4000 (the whole image: what a tracker's first frame asks for, so the slot is sized by it), 17 x 4000 (whole
    image) and 480 x 752 (a tracked ROI) with a camera each: every item against the oracle's chain."""
    s = _scene(orc)
    K, D, M = s["K"], s["D"], s["markers"]
    Ph = mpe.demo_params()
    n_pose = 0
    for i in range(2):
        pred = synth.project(s["T_true"][i], M, K) + np.random.default_rng(i).normal(0, 0.8, (5, 2))
        roi = orc.determine_roi(pred, ROWS, COLS, 20, K, D)
        assert roi[0] >= COLS // 2 - 40 and roi[1] >= ROWS // 2 - 40, roi
        r = hip.track_step(s["frames"][i], roi, Ph, K, D, M, pred)
        und, corr, ok, T = _oracle_track(orc, s["frames"][i], roi, K, D, M, pred, Ph.nearest_neighbour_pixel_tolerance)
        assert r["det_status"] == 0 and r["undist"].tobytes() == und.tobytes() and len(und) == 5, (i, roi)
        assert np.array_equal(r["corr"], corr) and (r["status"] == 0) == ok, i
        if ok:
            dp, dr = pose_diff(r["T"], T)
            assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (i, dp, dr)
            n_pose += 1
    assert n_pose == 2
    strip = fsc.frame(17, 4000, True)["img"]
    c2 = synth.make_frames("C2", 1, seed=321)
    pred2 = synth.project(c2["T_true"][0], c2["markers"], c2["K"]) + 0.4
    imgs = [s["frames"][1], np.ascontiguousarray(strip), c2["frames"][0]]
    cams = [(K, D), synth.camera_for(17, 4000), (c2["K"], c2["D"])]
    rois = [(0, 0, COLS, ROWS), (0, 0, 4000, 17), orc.determine_roi(pred2, 480, 752, 20, c2["K"], c2["D"])]
    preds = [None, None, pred2]
    setups = [(M, k, d, mpe.demo_params()) for k, d in cams]
    order = [2, 0, 1]              # the items are not listed by size
    dets, corr, res = hip.track_step_batch_formats([imgs[j] for j in order], [rois[j] for j in order],
                                                   [preds[j] for j in order], setups, order)
    posed = [_check_item(orc, dets[k], corr[k], res[k], imgs[j], rois[j], cams[j][0], cams[j][1], M, preds[j], j)
             for k, j in enumerate(order)]
    assert posed == [True, False, False] and dets["n"][1] == 5 and dets["n"][2] >= 7, (posed, dets["n"])


@pytest.mark.gpu
@pytest.mark.parametrize("encoding,rows", [("bgr8", 17), ("bayer_rggb8", 16), ("bayer_gbrg8", 16)])
def test_device_frames_of_4000_columns_in_the_cameras_encoding(hip, orc, encoding, rows):
    """One device-frame stream of 4000 columns in bgr8 and in two Bayer patterns (16 rows: a Bayer frame has even sides):
    the gather and decode kernels see x up to 3999 behind ROI origins beyond 2048.  Reference for the decoded bytes: the
    oracle's conversion (bgr8), the numpy witness (Bayer); for the detections: the oracle on those bytes."""
    import torch
    import witness_sensor_encodings as wit
    from test_encoded_device_streams import _encode
    cols = 4000
    gray = np.ascontiguousarray(fsc.frame(17, cols, True)["img"][17 - rows:])
    if encoding == "bgr8":
        raw = _encode(gray, encoding, False, 9)
        mono = orc.convert_to_mono8(raw, encoding)
    else:
        raw = wit.mosaic(gray, encoding, 9)
        mono = wit.to_mono8(raw, encoding)
    dev = torch.from_numpy(raw).cuda()
    conv = hip.convert_to_mono8(dev[None], encoding)
    assert np.array_equal(conv[0].cpu().numpy(), mono)
    K, D = synth.camera_for(rows, cols)
    rois = [(0, 0, cols, rows), (2049, 1, cols - 2049, rows - 1), (3071, 0, 929, rows), (cols - 17, rows - 9, 17, 9)]
    setups = [(synth.M5, K, D, mpe.demo_params())]
    dets, _, _ = hip.track_step_batch_device([dev] * len(rois), rois, [None] * len(rois), setups, None, encoding=encoding)
    n = 0
    for k, roi in enumerate(rois):
        und, dist = orc.find_leds(mono, orc.make_params(), K, D, roi=roi)
        _same_detections(dets[k], und, dist, (encoding, roi))
        n += len(und)
    assert n >= 8, n


@pytest.mark.gpu
def test_frames_and_windows_of_one_to_three_rows(hip, orc):
    """The other end of make_geom: there is no smallest frame.  The last 1, 2 and 3 rows of the salted 17 x 4000 strip and
    of 17 x 1982 as whole frames (detect_batch, detect_batch_wide, estimate_batch: no pose, the oracle's count) and as
    ROIs of ONE lock-step call (detection-only items) and of mpe_track_step: the oracle's detections to the bit, under
    the demo filter and wide open (a one-row window's contours have no area: none passes either)."""
    P_open = dict(min_blob_area=0.0, max_blob_area=1e9, max_width_height_distortion=1e9, max_circular_distortion=1e9)
    n = 0
    for rows, cols, clutter in ((17, 4000, True), (17, 1982, False)):
        img = fsc.frame(rows, cols, clutter)["img"]
        K, D = synth.camera_for(rows, cols)
        rois = [(0, rows - h, cols, h) for h in (1, 2, 3)] + [(cols // 2 + 1, rows - 2, cols - cols // 2 - 1, 2)]
        for kw in ({}, P_open):
            Po, Ph = orc.make_params(**kw), mpe.demo_params(**kw)
            refs = [orc.find_leds(img, Po, K, D, roi=r) for r in rois]
            if kw:      # (0 / 0 centroids of contours without area would not compare as bytes; there are none to compare)
                assert all(np.isfinite(u).all() for u, _ in refs)
            dets, _, _ = hip.track_step_batch([img] * len(rois), rois, [None] * len(rois), [(synth.M5, K, D, Ph)], [0] * len(rois))
            for k, roi in enumerate(rois):
                _same_detections(dets[k], *refs[k], (rows, cols, roi, "lock step"))
                r = hip.track_step(img, roi, Ph, K, D, synth.M5, np.full((5, 2), -1e6))
                assert r["det_status"] == 0 and r["undist"].tobytes() == refs[k][0].tobytes() and r["status"] == 1, (roi, "track_step")
                n += len(refs[k][0])
            for h in (1, 2, 3):
                part = np.ascontiguousarray(img[rows - h:])
                und, dist = orc.find_leds(part, Po, K, D)
                _same_detections(hip.detect_batch(part[None], K, D, Ph)[0], und, dist, (rows, cols, h, "detect_batch"))
                _same_detections(hip.detect_batch_wide(part[None], K, D, Ph)[0], und, dist, (rows, cols, h, "wide"))
                rec = hip.estimate_batch(part[None], synth.M5, K, D, Ph)[0]
                assert rec["status"] == 1 and rec["n_det"] == len(und), (rows, cols, h, int(rec["status"]), int(rec["n_det"]))
    assert n >= 4, n


# ---- GPU tier: the refusals ----------------------------------------------------------------------------------------------

def _refused(call, code=MPE_ERR_UNSUPPORTED, text="frame size unsupported"):
    with pytest.raises(mpe.MpeError) as e:
        call()
    assert "(%d)" % code in str(e.value) and text in str(e.value), str(e.value)


@pytest.mark.gpu
def test_frames_beyond_the_capacity_are_refused_by_every_entry(orc):
    """4097 rows and 4001 columns through every public entry that reaches make_geom — detect, ROI, estimate, wide,
    tracked, lock-step, tracker: MPE_ERR_UNSUPPORTED, "frame size unsupported"; 4096 rows and 4000 columns are taken;
    and the handle answers an ordinary call after every refusal exactly as a fresh handle does."""
    import torch
    tall, wide = np.zeros((fsc.MAX_ROWS + 1, 33), np.uint8), np.zeros((17, fsc.MAX_COLS + 1), np.uint8)
    K, D = synth.camera_for(480, 752)
    M, P = synth.M5, mpe.demo_params()
    probe = fsc.frame(17, 1982)["img"][None]
    Kp, Dp = synth.camera_for(17, 1982)
    fresh = mpe.Handle()
    want = fresh.detect_batch(probe, Kp, Dp, P).tobytes()
    fresh.close()
    und, dist = _ref(orc, (17, 1982, False), probe[0], Kp, Dp)
    h = mpe.Handle()
    t = mpe.Tracker(h, M, K, D, P)
    t2 = mpe.Tracker(h, M, K, D, P)
    res = torch.zeros(mpe.RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    try:
        n = 0
        for img in (tall, wide):
            rows, cols = img.shape
            full = (0, 0, cols, rows)
            su = [(M, K, D, P)]
            # (device frames: packed rows of a multiple of 16 bytes, or the entry answers for the layout first)
            dimg = torch.zeros((rows, 48) if img is tall else (16, fsc.MAX_COLS + 16), dtype=torch.uint8, device="cuda")
            dfull = (0, 0, dimg.shape[1], dimg.shape[0])
            calls = [lambda: h.detect_batch(img[None], K, D, P),
                     lambda: h.detect_batch_wide(img[None], K, D, P),
                     lambda: h.find_leds(img, P, K, D),
                     lambda: h.find_leds(img, P, K, D, roi=full),
                     lambda: h.estimate_batch(img[None], M, K, D, P),
                     lambda: h.estimate_batch_wide(img[None], M, K, D, P),
                     lambda: h.estimate_batch(dimg[None], M, K, D, P),
                     lambda: h.estimate_batch_device(dimg.data_ptr(), 1, dimg.shape[0], dimg.shape[1], M, K, D, P, res.data_ptr()),
                     lambda: h.track_step(img, full, P, K, D, M, np.zeros((5, 2))),
                     lambda: h.track_step_batch([img], [full], [None], su, [0]),
                     lambda: h.track_step_batch_wide([img], [full], [None], su, [0]),
                     lambda: h.track_step_batch_device([dimg], [dfull], [None], su, None),
                     lambda: h.track_step_batch_formats([img, probe[0]], [full, (0, 0, 1982, 17)], [None, None], su, None),
                     lambda: t.estimate(img, 0.0),
                     lambda: mpe.tracker_estimate_batch([t, t2], [img, img], [0.0, 0.0]),
                     lambda: mpe.tracker_estimate_batch_mixed([t, t2], [img, img], [0.0, 0.0]),
                     lambda: mpe.tracker_estimate_batch_device([t, t2], [dimg, dimg], [0.0, 0.0]),
                     lambda: mpe.tracker_estimate_batch_formats([t, t2], [img, probe[0]], [0.0, 0.0])]
            for k, call in enumerate(calls):
                _refused(call)
                assert h.detect_batch(probe, Kp, Dp, P).tobytes() == want, (img.shape, k)
                n += 1
        assert n == 36
        _same_detections(np.frombuffer(want, mpe.DETECTIONS_DTYPE)[0], und, dist, "probe")
        # each axis at its cap is taken (both at once: test_detection_and_rois_on_the_full_size_frame)
        for rows, cols in ((fsc.MAX_ROWS, 33), (17, fsc.MAX_COLS)):
            img = fsc.frame(rows, cols)["img"]
            Kc, Dc = synth.camera_for(rows, cols)
            _same_detections(h.detect_batch(img[None], Kc, Dc, P)[0], *_ref(orc, (rows, cols, False), img, Kc, Dc), (rows, cols))
            assert not t.estimate(img, 0.0)["updated"]           # (no marker set in sight: no pose, and no error)
            t.reset()
    finally:
        t.close()
        t2.close()
        h.close()


@pytest.mark.gpu
def test_lds_budget_decides_which_widths_are_taken(orc):
    """Option "lds_budget": 8191 and 160 KiB + 1 are MPE_ERR_ARG; at 8192 a 17 x 4000 frame is refused (5 bitmap rows
    fit, fewer than the 8 make_geom needs — fsc.slot_cap restates the arithmetic) while 17 x 752 is taken; at the
    default both are taken, with the oracle's detections."""
    P = mpe.demo_params()
    big, small = fsc.frame(17, 4000)["img"], np.ascontiguousarray(fsc.frame(17, 4000)["img"][:, :752])
    Kb, Db = synth.camera_for(17, 4000)
    Ks, Ds = synth.camera_for(17, 752)
    assert fsc.slot_cap(17, 4000, 8192) < 8 <= fsc.slot_cap(17, 752, 8192) and fsc.slot_cap(17, 4000, 64 * 1024) >= 8
    h = mpe.Handle()
    try:
        assert h.get_option("lds_budget") == 64 * 1024
        for bad in (8191, 160 * 1024 + 1):
            _refused(lambda: h.set_option("lds_budget", bad), MPE_ERR_ARG, "lds_budget out of range")
            assert h.get_option("lds_budget") == 64 * 1024
        h.set_option("lds_budget", 8192)
        _refused(lambda: h.detect_batch(big[None], Kb, Db, P))
        _refused(lambda: h.find_leds(big, P, Kb, Db))
        _same_detections(h.detect_batch(small[None], Ks, Ds, P)[0], *orc.find_leds(small, orc.make_params(), Ks, Ds), "small, 8192")
        h.set_option("lds_budget", 64 * 1024)
        _same_detections(h.detect_batch(big[None], Kb, Db, P)[0], *_ref(orc, (17, 4000, False), big, Kb, Db), "big, default")
        _same_detections(h.detect_batch(small[None], Ks, Ds, P)[0], *orc.find_leds(small, orc.make_params(), Ks, Ds), "small, default")
    finally:
        h.close()
