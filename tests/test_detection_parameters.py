"""The two pieces of the blob kernel every detection entry goes through — blob_filter and undistort_point
(csrc/mpe_k1b_dev.h) — where they decide something: every predicate of the shape filter exactly on its edge, and the
rational distortion model with 0, 4, 5, 8 and 12 coefficients and a skewed K.  The inputs and the float64 statistics come
from tests/detection_parameter_cases.py; the reference is the CPU oracle, which the CPU tier below first checks against
those statistics so that no case is vacuous.  (The host build of the device source runs the same points in
tests/test_k1b_host.py.)"""
import numpy as np
import pytest

import rpg_monocular_pose_estimator_amd as mpe
from rpg_monocular_pose_estimator_amd import synth
import detection_parameter_cases as dpc
import witness_rig
from util import pose_diff, POS_TOL_M, ROT_TOL_RAD

FRAME_KW = dict(threshold_value=dpc.THR, gaussian_sigma=dpc.SIGMA)
PAD_X, PAD_Y = 7, 5      # the ROI's odd origin inside the padded frame


@pytest.fixture(scope="module")
def shapes(orc):
    img = dpc.shape_frame()
    stats = dpc.contour_statistics(orc, img)
    padded = np.ascontiguousarray(np.pad(img, ((PAD_Y, 3), (PAD_X, 9))))
    return dict(img=img, stats=stats, points=dpc.parameter_points(stats), padded=padded,
                roi=(PAD_X, PAD_Y, dpc.COLS, dpc.ROWS), camera=synth.camera_for(*padded.shape))


def _same_detections(rec, und, dist, what):
    """One detection record of the library against the oracle's lists: count, order, bytes."""
    n = len(und)
    assert rec["status"] == 0 and rec["n"] == n, (what, int(rec["status"]), int(rec["n"]), n)
    assert rec["dist_xy"][:2 * n].tobytes() == np.ascontiguousarray(dist, np.float32).tobytes(), what
    assert rec["undist_xy"][:2 * n].tobytes() == np.ascontiguousarray(und, np.float64).tobytes(), what


# ---- CPU tier --------------------------------------------------------------------------------------------------------

def test_shape_frame_has_what_the_tests_need(orc, shapes):
    """The requirements on the drawn frame, so that a later edit cannot empty the tests: six or more contours, one with
    a hole (the literal border trace), three or more without (the cell sums), both bar orientations (the width and the
    height test disagree, each way round), odd and even widths; the sigma-0.2 frame holds blobs of width 1 and height 1
    whose integer half is 0."""
    st = shapes["stats"]
    assert len(st) >= 6
    assert sum(s["hole"] for s in st) >= 1 and sum(not s["hole"] for s in st) >= 3
    assert any(s["w"] > 2 * s["h"] and s["circ_h"] > 2 * s["circ_w"] for s in st)       # a wide bar: the height test binds
    assert any(s["h"] > 2 * s["w"] and s["circ_w"] > 2 * s["circ_h"] for s in st)       # a tall bar: the width test binds
    assert any(s["w"] % 2 for s in st) and any(s["w"] % 2 == 0 for s in st)
    assert all(float(s["area"] * 2) == int(s["area"] * 2) for s in st)                  # exact half-integers
    thin = dpc.contour_statistics(orc, dpc.thin_frame(), sigma=0.2)
    assert list(orc.gaussian_kernel_q8(0.2)) == [0, 256, 0]
    assert any(s["w"] == 1 and s["h"] > 1 for s in thin) and any(s["h"] == 1 and s["w"] > 1 for s in thin)
    assert all(np.isnan(s["circ"]) for s in thin if min(s["w"], s["h"]) == 1)


def test_oracle_drops_exactly_the_contours_on_each_edge(orc, shapes):
    """At every (predicate, statistic) the oracle keeps the contour at the statistic itself and drops it one float64
    further, together with exactly those that share the statistic — and its count at either value is the one the float64
    statistics predict.  Drop per edge (area 8, 41, 56, 76, 108, 168, 217; width/height 0, 0.3077, 0.5333; circular
    0.0793 .. 1.688): min area 1 1 1 2 1 1 1, max area 1 1 1 2 1 1 1, width/height 5 1 2, circular 1 1 1 1 1 1 2."""
    K, D = shapes["camera"]
    edges = dpc.edge_points(shapes["stats"])
    assert sum(e[4] for e in edges) == 4 * len(shapes["stats"]) == 32     # every contour sits on one edge per predicate
    drops = []
    for label, field, keep, drop, share in edges:
        n = []
        for v in (keep, drop):
            kw = dict(dpc.OPEN, **{field: v})
            n.append(len(orc.find_leds(shapes["img"], orc.make_params(**kw, **FRAME_KW), K, D)[1]))
            assert n[-1] == dpc.expected_count(shapes["stats"], kw), (label, v, n)
        assert n[0] - n[1] == share >= 1, (label, n, share)
        drops.append(share)
    assert drops == [1, 1, 1, 2, 1, 1, 1] * 2 + [5, 1, 2] + [1, 1, 1, 1, 1, 1, 2], drops
    for mc in (1e9, float("inf")):    # width 1: |1 - 0 / 0| is never <= anything, inf included
        P = orc.make_params(**dict(dpc.OPEN, max_circular_distortion=mc, threshold_value=dpc.THR, gaussian_sigma=0.2))
        assert len(orc.find_leds(dpc.thin_frame(), P, K, D)[1]) == 1, mc


def test_rational_scenes_are_posed_by_the_oracle(orc):
    """The precondition of the full-pipeline GPU checks: the oracle has a pose on at least 6 of the 8 frames of every
    camera and on at least 9 of the 12 tracked frames (the reference places its ROI with the polynomial model only)."""
    for name in ("D4", "D5", "D8"):
        assert int((_estimate_case(orc, name)["ref"]["status"] == 0).sum()) >= 6, name
    assert sum(r["updated"] for r in _tracked_case(orc)["ref"]) >= 9


_CASES = {}
# The body anywhere in the image, not only near its centre: on these frames zeroing k3, k4 or k5 of D8 alone moves the
# oracle's pose by 0.34 mm, 203 mm (and loses three of eight poses) and 3.2 mm — more than the pose tolerance — while the
# reference's polynomial-only ROI placement still finds every LED.
SPREAD = dict(lateral=(0.45, 0.28), depth=(0.9, 1.5), margin=30.0)


def _estimate_case(orc, name):
    if ("est", name) not in _CASES:
        K, D = dpc.CAMERAS[name]
        frames, _ = dpc.rational_frames(8, 300, K, D, **SPREAD)
        ref = orc.estimate_batch(frames, synth.M5, K, D, orc.make_params(), n_threads=4)
        _CASES["est", name] = dict(frames=frames, K=K, D=D, ref=ref)
    return _CASES["est", name]


def _tracked_case(orc):
    if "seq" not in _CASES:
        K, D = dpc.CAMERAS["D8"]
        q = dpc.rational_sequence(12, 78, [(K, D)], **SPREAD)
        t = orc.Tracker(q["markers"], K, D, orc.make_params())
        ref = [t.estimate(q["frames"][0][k], q["times"][k]) for k in range(12)]
        t.close()
        _CASES["seq"] = dict(q=q, K=K, D=D, ref=ref)
    return _CASES["seq"]


# ---- GPU tier: the shape filter --------------------------------------------------------------------------------------

@pytest.fixture(params=[0, 1], ids=["general_slabs", "general_lds"])
def general_tier(request, hip):
    """Both kernels of the general blob tier: k1b_general (bitmaps in global-memory slabs) and k1b_general_lds (a block
    per CU, the frame's bitmaps in LDS)."""
    hip.set_option("general_lds", request.param)
    yield request.param
    hip.set_option("general_lds", 0)


@pytest.mark.gpu
def test_filter_edges_in_the_lds_tiers(hip, orc, shapes):
    """mpe_detect_batch (the padded frame and its 180-degree turn) and mpe_find_leds (a ROI with an odd origin) at every
    parameter point of the edge table: the oracle's detections, byte for byte."""
    K, D = shapes["camera"]
    frames = np.ascontiguousarray(np.stack([shapes["padded"], shapes["padded"][::-1, ::-1]]))
    for label, kw in shapes["points"]:
        Po, Ph = orc.make_params(**kw, **FRAME_KW), mpe.demo_params(**kw, **FRAME_KW)
        got = hip.detect_batch(frames, K, D, Ph)
        for i, f in enumerate(frames):
            und, dist = orc.find_leds(f, Po, K, D)
            assert len(und) == dpc.expected_count(shapes["stats"], kw), label
            _same_detections(got[i], und, dist, (label, i))
        und, dist = orc.find_leds(shapes["padded"], Po, K, D, roi=shapes["roi"])
        uh, dh = hip.find_leds(shapes["padded"], Ph, K, D, roi=shapes["roi"])
        assert dh.tobytes() == dist.tobytes() and uh.tobytes() == und.tobytes(), label
    thin = dpc.thin_frame()
    for mc in (1e9, float("inf")):
        kw = dict(dpc.OPEN, max_circular_distortion=mc, threshold_value=dpc.THR, gaussian_sigma=0.2)
        und, dist = orc.find_leds(thin, orc.make_params(**kw), K, D, roi=(3, 1, 59, 30))
        uh, dh = hip.find_leds(thin, mpe.demo_params(**kw), K, D, roi=(3, 1, 59, 30))
        assert len(und) == 1 and dh.tobytes() == dist.tobytes() and uh.tobytes() == und.tobytes(), mc
        _same_detections(hip.detect_batch(thin[None], K, D, mpe.demo_params(**kw))[0], *orc.find_leds(thin, orc.make_params(**kw), K, D), mc)


def _general_points(shapes):
    """Eight parameter points for the general tier: the bars' edges (width against height), an area edge two contours
    share, the ellipse's, a mixed point and the demo point."""
    want = ("max_circular_distortion@1.6879501499964547:keep", "max_circular_distortion@1.6879501499964547:drop",
            "max_circular_distortion@0.5048512881585479:drop", "max_width_height_distortion@0.5333333333333333:drop",
            "min_blob_area@76.0:keep", "max_blob_area@76.0:drop", "mixed:circ+wh", "demo")
    pts = dict(shapes["points"])
    return [(k, pts[k]) for k in want]


@pytest.fixture(scope="module")
def cluttered(orc, shapes):
    frames = dpc.cluttered_shape_frames(64, 5)
    K, D = synth.camera_for(*frames.shape[1:])
    ref = {label: [orc.find_leds(f, orc.make_params(**kw, **FRAME_KW), K, D) for f in frames]
           for label, kw in _general_points(shapes)}
    return dict(frames=frames, K=K, D=D, ref=ref)


@pytest.mark.gpu
def test_filter_edges_in_the_general_tier(hip, orc, shapes, cluttered, general_tier):
    """The same shapes above a column of 38 one-pixel bands — more bands than either LDS tier takes — in a batch of 64
    frames, under both kernels of the general tier, at eight parameter points.  The read-out "general_seen" (frames the
    last batch handed to the general tier) confirms where they ran."""
    frames, K, D = cluttered["frames"], cluttered["K"], cluttered["D"]
    kept = set()
    for label, kw in _general_points(shapes):
        got = hip.detect_batch(frames, K, D, mpe.demo_params(**kw, **FRAME_KW))
        assert hip.get_option("general_seen") == len(frames), (label, hip.get_option("general_seen"))
        for i, (und, dist) in enumerate(cluttered["ref"][label]):
            _same_detections(got[i], und, dist, (label, general_tier, i))
        kept.add(len(cluttered["ref"][label][0][0]))
    assert len(kept) >= 5, kept       # the points differ in what they keep


@pytest.mark.gpu
def test_lock_step_setups_that_differ_in_one_filter_field(hip, orc, shapes):
    """ONE mpe_track_step_batch_setups call whose set-ups — one per parameter point of the edge table, some fifty — share
    camera, markers, threshold and sigma and differ only in a filter field; every item looks at the same frame through
    the same ROI (odd origin).  Every item's detections are the oracle's for its own set-up: a filter value read from a
    neighbour's entry of the per-set-up table shows as a wrong count."""
    K, D = shapes["camera"]
    pts = shapes["points"]
    setups = [(synth.M5[:4], K, D, mpe.demo_params(**kw, **FRAME_KW)) for _, kw in pts]
    n = len(pts)
    assert n >= 4
    order = list(np.random.default_rng(3).permutation(n))     # items are not listed in the order of their set-ups
    dets, corr, res = hip.track_step_batch([shapes["padded"]] * n, [shapes["roi"]] * n, [None] * n, setups, order)
    counts = set()
    for i, s in enumerate(order):
        label, kw = pts[s]
        und, dist = orc.find_leds(shapes["padded"], orc.make_params(**kw, **FRAME_KW), K, D, roi=shapes["roi"])
        _same_detections(dets[i], und, dist, (label, i))
        counts.add(len(und))
    assert counts >= set(range(0, 9)), counts                   # every count from none to all eight occurs


@pytest.mark.gpu
def test_wide_entry_with_a_filter_that_is_not_the_demos(hip, orc):
    """mpe_track_step_batch_wide on the 70-spot grid frame of test_wide_frames.  Its spots all have the same statistics
    (area 48, 8 x 9), so the filter is closed down ONTO them — all four fields at the spots' own values: every one of
    the 70 is kept, as the oracle keeps them, and none once the circular bound is one float64 lower (the second set-up
    of the same call)."""
    from test_wide_frames import grid_frame, GRID_ROWS, GRID_COLS
    K, D = synth.camera_for(GRID_ROWS, GRID_COLS)
    frame = grid_frame(np.random.default_rng(70), 70)
    st = dpc.contour_statistics(orc, frame)
    assert len(st) == 70 and len({(float(s["area"]), float(s["wh"]), float(s["circ"])) for s in st}) == 1
    on = dict(min_blob_area=float(st[0]["area"]), max_blob_area=float(st[0]["area"]),
              max_width_height_distortion=float(st[0]["wh"]), max_circular_distortion=float(st[0]["circ"]), **FRAME_KW)
    off = dict(on, max_circular_distortion=float(np.nextafter(st[0]["circ"], 0.0)))
    und, dist = orc.find_leds(frame, orc.make_params(**on), K, D)
    assert mpe.MAX_DETECTIONS < len(und) == 70 and len(orc.find_leds(frame, orc.make_params(**off), K, D)[0]) == 0
    roi = (0, 0, GRID_COLS, GRID_ROWS)
    setups = [(synth.M5[:4], K, D, mpe.demo_params(**on)), (synth.M5[:4], K, D, mpe.demo_params(**off))]
    dets, corr, res = hip.track_step_batch_wide([frame, frame], [roi, roi], [None, None], setups, [0, 1])
    _same_detections(dets[0], und, dist, "wide, on the edge")
    assert dets["n"][1] == 0 and dets["status"][1] == 0


# ---- GPU tier: the distortion models ---------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(dpc.CAMERAS))
def test_detection_with_every_distortion_model(hip, orc, name):
    """mpe_detect_batch and mpe_find_leds (ROI) with 0, 4, 5, 8 and 12 coefficients and a skewed K on frames of spots far
    from the principal point: dist_xy and undist_xy are the oracle's bytes."""
    K, D = dpc.CAMERAS[name]
    rng = np.random.default_rng(60 + list(dpc.CAMERAS).index(name))
    frames = np.stack([dpc.spots_frame(rng, K, D) for _ in range(3)])
    Po, Ph = orc.make_params(), mpe.demo_params()
    got = hip.detect_batch(frames, K, D, Ph)
    n = 0
    for i, f in enumerate(frames):
        und, dist = orc.find_leds(f, Po, K, D)
        _same_detections(got[i], und, dist, (name, i))
        roi = (11, 3, 180, 110)
        und, dist = orc.find_leds(f, Po, K, D, roi=roi)
        uh, dh = hip.find_leds(f, Ph, K, D, roi=roi)
        assert dh.tobytes() == dist.tobytes() and uh.tobytes() == und.tobytes(), (name, i)
        n += len(und)
    assert n >= 15, n
    if name == "D12":      # ... and behaves as its first eight coefficients
        again = hip.detect_batch(frames, K, dpc.D8, Ph)
        for i in range(len(frames)):
            k = 2 * int(got["n"][i])
            assert again["n"][i] == got["n"][i] and again["undist_xy"][i][:k].tobytes() == got["undist_xy"][i][:k].tobytes(), i


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["D4", "D5", "D8"])
def test_estimate_batch_with_every_distortion_model(hip, orc, name):
    """mpe_estimate_batch on 8 C2 frames rendered through the forward rational model: status, n_det, n_corr and the pose
    (tolerance of test_gpu_parity.test_estimate_batch_parity) against the oracle."""
    c = _estimate_case(orc, name)
    ro = c["ref"]
    rh = hip.estimate_batch(c["frames"], synth.M5, c["K"], c["D"], mpe.demo_params())
    assert int((ro["status"] == 0).sum()) >= 6
    assert np.array_equal(rh["status"], ro["status"]) and np.array_equal(rh["n_det"], ro["n_det"])
    assert np.array_equal(rh["n_corr"], ro["n_corr"])
    for i in range(8):
        if ro["status"][i] == 0:
            dp, dr = pose_diff(rh["T"][i], ro["T"][i])
            assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (name, i, dp, dr)


def _check_tracked(out, ro, what):
    """One frame's record of mpe.Tracker.estimate against orc.Tracker.estimate."""
    assert out["updated"] == ro["updated"] and out["roi"] == ro["roi"], (what, out["roi"], ro["roi"])
    assert out["it_since_initialized"] == ro["it_since_initialized"] and out["n_det"] == ro["n_det"], what
    assert out["n_corr"] == ro["n_corr"] and out["used_bruteforce"] == ro["used_bruteforce"], what
    if ro["updated"]:
        dp, dr = pose_diff(out["T"], ro["T"])
        assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (what, dp, dr)


@pytest.mark.gpu
def test_tracked_sequence_with_eight_coefficients(hip, orc):
    """12 frames through mpe.Tracker with D8 against orc.Tracker: ROI, counters, branch and pose of every frame, and the
    undistorted image points of the last detection bit for bit."""
    c = _tracked_case(orc)
    q, K, D = c["q"], c["K"], c["D"]
    assert sum(r["updated"] for r in c["ref"]) >= 9
    t = mpe.Tracker(hip, q["markers"], K, D, mpe.demo_params())
    try:
        for k in range(12):
            out = t.estimate(q["frames"][0][k], q["times"][k])
            _check_tracked(out, c["ref"][k], k)
            und, _ = orc.find_leds(q["frames"][0][k], orc.make_params(), K, D, roi=out["roi"])
            assert t.image_points().tobytes() == und.tobytes(), k
    finally:
        t.close()


@pytest.mark.gpu
def test_rig_step_with_one_eight_coefficient_camera(hip, orc):
    """A two-camera rig through Rig.step, camera 1 with D8: each camera's records against its own orc.Tracker, and the
    rig record is mpe_rig_optimise_pose_batch over the rows read back through the getters, near the true pose."""
    K0, D0 = synth.camera_for(480, 752)
    cams = [(K0, D0), dpc.CAMERAS["D8"]]
    E = np.array([np.eye(4), np.eye(4)])
    E[1][:3, :3] = synth.rodrigues([0.1, 1.0, 0.05], -0.04)
    E[1][:3, 3] = [-0.06, 0.01, 0.005]
    q = dpc.rational_sequence(6, 91, cams, E)
    ts = [mpe.Tracker(hip, q["markers"], K, D, mpe.demo_params()) for K, D in cams]
    refs = [orc.Tracker(q["markers"], K, D, orc.make_params()) for K, D in cams]
    rig = mpe.Rig(hip, ts, E)
    own, fused_err = [], []
    try:
        for k in range(6):
            imgs = [f[k] for f in q["frames"]]
            rec, info, upd, rr, fused = rig.step(imgs, [q["times"][k]] * 2)
            rows = []
            for c, t in enumerate(ts):
                ro = refs[c].estimate(imgs[c], q["times"][k])
                own.append(float(np.linalg.norm((ro["T"] - q["T_true_cam"][c][k])[:3, 3])))
                assert bool(upd[c]) == ro["updated"] and tuple(info[c, 0:4]) == ro["roi"], (k, c)
                assert info[c, 5] == ro["n_det"] and info[c, 6] == ro["n_corr"] and bool(info[c, 7]) == ro["used_bruteforce"], (k, c)
                if ro["updated"]:
                    dp, dr = pose_diff(rec["T"][c].reshape(4, 4), ro["T"])
                    assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (k, c, dp, dr)
                und, _ = orc.find_leds(imgs[c], orc.make_params(), cams[c][0], cams[c][1], roi=ro["roi"])
                xy = t.image_points()
                assert xy.tobytes() == und.tobytes(), (k, c)
                if upd[c]:
                    rows += [(c, q["markers"][m - 1], xy[j - 1]) for m, j in t.correspondences()]
            assert upd.all() and fused, k
            cameras = [(K, E[c]) for c, (K, _) in enumerate(cams)]
            again = hip.rig_optimise_pose_batch(cameras, [rows], [rec["T"][0].reshape(4, 4)])
            assert again.tobytes() == rr.tobytes(), k
            witness_rig.check_against_witness(rr[0], cameras, rows, rec["T"][0].reshape(4, 4), k)
            fused_err.append(float(np.linalg.norm((rr["T"][0].reshape(4, 4) - q["T_true"][k])[:3, 3])))
        # against the truth: the oracle's own single-camera poses are up to 8 mm off in depth on this sequence (the
        # centroid noise of 1.5-px spots at 1.4 m); the joint fit over both cameras' rows is never further off than
        # the worst of them
        assert max(fused_err) <= max(own), (fused_err, own)
    finally:
        for t in ts:
            t.close()
        for r in refs:
            r.close()


# ---- GPU tier: set-ups that differ in one number -----------------------------------------------------------------------

def _one_number_apart(orc):
    """(what, D of stream 0, D of stream 1, parameters of stream 0, of stream 1, frames, times): streams over the SAME
    frames whose set-ups differ in D[7], in D[4] or in max_circular_distortion alone.  The body is rendered through D8
    anywhere in the image, so that k6 matters; the circular bound sits on one LED's own statistic in stream 0 and one
    float64 below it in stream 1."""
    K = synth.README_K
    q = dpc.rational_sequence(6, 55, [(K, dpc.D8)], lateral=(0.3, 0.2), depth=(0.9, 1.4), margin=25.0)
    frames = q["frames"][0]
    D7, D4_ = dpc.D8.copy(), dpc.D8.copy()
    D7[7] = 0.0
    D4_[4] = -0.02
    st = dpc.contour_statistics(orc, frames[0])
    assert len(st) == 5
    mc = max(float(s["circ"]) for s in st)
    assert mc < 0.5
    return q, [("D[7]", dpc.D8, D7, {}, {}), ("D[4]", dpc.D8, D4_, {}, {}),
               ("max_circular_distortion", dpc.D8, dpc.D8, dict(max_circular_distortion=mc),
                dict(max_circular_distortion=float(np.nextafter(mc, 0.0))))]


@pytest.mark.gpu
def test_trackers_one_number_apart_are_two_setups(hip, orc):
    """Two trackers on one handle over the same frames, their set-ups differing in one number: the uniform lock-step entry
    refuses the pair (MPE_ERR_ARG, as for any mixed group), the mixed entry answers each stream with its own oracle's
    record — and the two streams' image points or counts do differ, so a shared set-up would show."""
    K = synth.README_K
    q, cases = _one_number_apart(orc)
    frames, times = q["frames"][0], q["times"]
    for what, Da, Db, kwa, kwb in cases:
        ts = [mpe.Tracker(hip, q["markers"], K, D, mpe.demo_params(**kw)) for D, kw in ((Da, kwa), (Db, kwb))]
        refs = [orc.Tracker(q["markers"], K, D, orc.make_params(**kw)) for D, kw in ((Da, kwa), (Db, kwb))]
        try:
            with pytest.raises(mpe.MpeError, match=r"mpe_tracker_estimate_batch failed \(-1\)"):
                mpe.tracker_estimate_batch(ts, [frames[0]] * 2, [times[0]] * 2)
            differ = False
            for k in range(len(frames)):
                rec, info, upd = mpe.tracker_estimate_batch_mixed(ts, [frames[k]] * 2, [times[k]] * 2)
                pts = []
                for c, (D, kw) in enumerate(((Da, kwa), (Db, kwb))):
                    ro = refs[c].estimate(frames[k], times[k])
                    assert bool(upd[c]) == ro["updated"] and tuple(info[c, 0:4]) == ro["roi"], (what, k, c)
                    assert info[c, 4] == ro["it_since_initialized"] and info[c, 5] == ro["n_det"], (what, k, c)
                    assert info[c, 6] == ro["n_corr"] and bool(info[c, 7]) == ro["used_bruteforce"], (what, k, c)
                    if ro["updated"]:
                        dp, dr = pose_diff(rec["T"][c].reshape(4, 4), ro["T"])
                        assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (what, k, c, dp, dr)
                    und, _ = orc.find_leds(frames[k], orc.make_params(**kw), K, D, roi=ro["roi"])
                    assert ts[c].image_points().tobytes() == und.tobytes(), (what, k, c)
                    pts.append(und.tobytes())
                differ = differ or pts[0] != pts[1]
            assert differ, what
        finally:
            for t in ts:
                t.close()
            for r in refs:
                r.close()


@pytest.mark.gpu
def test_detect_batch_carries_nothing_over_between_calls(hip, orc):
    """On one handle, with the same K: mpe_detect_batch, then again with D[6] alone changed, then with min_blob_area alone
    changed — every call's answer is the oracle's for that call's values, and differs from the call before."""
    K = synth.README_K
    rng = np.random.default_rng(66)
    frames = np.stack([dpc.spots_frame(rng, K, dpc.D8) for _ in range(2)])
    st = dpc.contour_statistics(orc, frames[0])
    areas = sorted(float(s["area"]) for s in st)
    D6 = dpc.D8.copy()
    D6[6] = 0.05
    calls = [(dpc.D8, {}), (D6, {}), (D6, dict(min_blob_area=float(np.nextafter(areas[len(areas) // 2], np.inf)))), (dpc.D8, {})]
    before = None
    for D, kw in calls:
        got = hip.detect_batch(frames, K, D, mpe.demo_params(**kw))
        now = b""
        for i, f in enumerate(frames):
            und, dist = orc.find_leds(f, orc.make_params(**kw), K, D)
            _same_detections(got[i], und, dist, (kw, i))
            now += und.tobytes()
        assert now != before
        before = now
