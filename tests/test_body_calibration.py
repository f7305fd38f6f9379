"""The LED positions of a body calibrated from the sequences it was tracked in, on the device (mpe_body_calibrate: the
k_body_ba_* kernels, Handle.body_calibrate, BodyCalibrator), at the smallest shapes at which the kernels can still go
wrong, against the numpy witness (tests/witness_body_ba.py) with its criteria: marker positions and view poses within
1e-9, covariance allclose(rtol=1e-5, atol=1e-12), iterations within +-1, states / counts / flags equal."""
import ctypes as C
import json

import numpy as np
import pytest

import rpg_monocular_pose_estimator_amd as mpe
from rpg_monocular_pose_estimator_amd import synth
import witness_body_ba as wbb

pytestmark = pytest.mark.gpu


def _calibrate(hip, prob, **kw):
    return hip.body_calibrate(prob["cameras"], prob["views"], prob["markers"], prob["T_start"], **kw)


def _same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("markers", "T_views", "cov", "view_used")) \
        and a["report"] == b["report"] and a["ok"] == b["ok"]


def test_one_camera_four_markers_six_views(hip):
    """The single-camera case: auto holds the scale, seven constraints on a 12 x 12 system."""
    prob = wbb.random_body_calibration(np.random.default_rng(41), 1, 6, 4, p_missing=0.0)
    got = _calibrate(hip, prob)
    assert got["ok"] and got["report"]["scale_held"] == 1 and got["report"]["rows_used"] == 24
    w = wbb.check_against_witness(got, prob, "1 x 4 x 6")
    assert w["report"]["iterations"] <= 10
    assert got["report"]["rms_after"] <= got["report"]["rms_before"]


def test_two_cameras_four_markers_two_views(hip):
    prob = wbb.random_body_calibration(np.random.default_rng(42), 2, 2, 4, p_missing=0.0)
    got = _calibrate(hip, prob)
    assert got["ok"] and got["report"]["scale_held"] == 0 and got["report"]["views_used"] == 2 and got["report"]["rows_used"] == 16
    w = wbb.check_against_witness(got, prob, "2 x 4 x 2")
    assert w["report"]["iterations"] <= 10


def test_sixteen_cameras_of_sixteen_markers(hip):
    """256 rows a view, a 48 x 48 reduced system, 136 blocks in the reduction: the caps of all three."""
    prob = wbb.random_body_calibration(np.random.default_rng(43), 16, 3, 16, p_missing=0.0)
    assert all(len(rows) == 256 for rows in prob["views"])
    got = _calibrate(hip, prob)
    assert got["ok"] and got["report"]["marker_state"] == [1] * 16 and got["report"]["rows_used"] == 768
    w = wbb.check_against_witness(got, prob, "16 x 16 x 3")
    assert w["report"]["iterations"] <= 10


@pytest.mark.parametrize("n_views", [65, 84, 300])
def test_view_counts_across_wave_block_and_chunk_boundaries(hip, n_views):
    """3 cameras of 5 markers, rows missing with probability 0.3: 65 views — one more than a wave has lanes and than an
    update block and a staging pass of the reduction hold —, 84 and 300 (four full passes and a partial one); then the
    same call with the records of only a few views on the device at a time (16 KiB: chunks of about nine views, the
    last one shorter): the same bits."""
    prob = wbb.random_body_calibration(np.random.default_rng(44 + n_views), 3, n_views, 5, p_missing=0.3)
    got = _calibrate(hip, prob)
    assert got["ok"] and got["report"]["views_used"] >= n_views - 2
    wbb.check_against_witness(got, prob, n_views)
    hip.set_option("rig_ba_record_kb", 16)
    try:
        assert hip.get_option("rig_ba_record_kb") == 16
        chunked = _calibrate(hip, prob)
    finally:
        hip.set_option("rig_ba_record_kb", 0)
    assert _same(chunked, got)


def test_held_markers_and_unused_views(hip):
    """A marker with one row, a marker without rows, a view of 3 rows and a view of 2 markers: the reported states and
    counts are the witness's, and what is not calibrated comes back as it went in, bit for bit."""
    prob = wbb.random_body_calibration(np.random.default_rng(45), 2, 14, 6, p_missing=0.0)
    views = [[r for r in rows if r[1] != 4 and (r[1] != 5 or (f == 2 and r[0] == 1))] for f, rows in enumerate(prob["views"])]
    views[6] = views[6][:3]
    views[10] = [r for r in views[10] if r[1] in (1, 3)]
    prob["views"] = views
    got = _calibrate(hip, prob)
    assert got["ok"] and got["report"]["marker_state"] == [1, 1, 1, 1, 2, 2] and got["report"]["marker_rows"][4:] == [0, 0]
    assert list(got["view_used"]) == [f not in (6, 10) for f in range(14)] and got["report"]["rows_used"] == 12 * 8
    wbb.check_against_witness(got, prob, "held and unused")
    for m in (4, 5):
        assert got["markers"][m].tobytes() == np.ascontiguousarray(prob["markers"][m]).tobytes(), m
        assert not got["cov"][m].any(), m
    unused = ~got["view_used"]
    assert got["T_views"][unused].tobytes() == np.ascontiguousarray(prob["T_start"][unused]).tobytes()
    # two markers in all: nothing is calibrated, everything comes back
    prob["views"] = [[r for r in rows if r[1] < 2] for rows in views]
    got = _calibrate(hip, prob)
    assert not got["ok"] and got["report"]["status"] == 1 and got["report"]["views_used"] == 0
    assert got["report"]["marker_state"] == [2] * 6 and not got["view_used"].any()
    assert got["T_views"].tobytes() == np.ascontiguousarray(prob["T_start"]).tobytes()
    assert got["markers"].tobytes() == np.ascontiguousarray(prob["markers"]).tobytes() and not got["cov"].any()
    wbb.check_against_witness(got, prob, "two markers")


def test_the_same_call_twice_gives_the_same_bits(hip):
    prob = wbb.random_body_calibration(np.random.default_rng(46), 4, 70, 5, p_missing=0.3)
    first = _calibrate(hip, prob, scale=1)
    rows = [(c, prob["markers"][m], uv) for c, m, uv in prob["views"][0]]
    hip.rig_optimise_pose_batch(prob["cameras"], [rows], [prob["T_start"][0]])   # (another user of the buffers)
    second = _calibrate(hip, prob, scale=1)
    assert first["ok"] and first["report"]["scale_held"] == 1 and _same(first, second)
    wbb.check_against_witness(first, prob, "scale held on a rig", scale=1)


def _raw(hip, prob, n_cameras=None, n_markers=None, begin=None, cam=None, mk=None, scale=-1, max_it=50, tol=1e-10, null=(),
         sentinel=0x5a):
    """mpe_body_calibrate through ctypes with one argument spoilt -> (rc, message, every output still the sentinel)"""
    lib = hip._lib
    cams, b, c, m, uv = mpe.pack_body_views(prob["cameras"] + [prob["cameras"][0]] * 16, prob["views"])
    n_cameras = len(prob["cameras"]) if n_cameras is None else n_cameras
    xyz = np.zeros((17, 3))
    xyz[:len(prob["markers"])] = prob["markers"]
    n_markers = len(prob["markers"]) if n_markers is None else n_markers
    b = b if begin is None else np.ascontiguousarray(begin, np.int32)
    c = c if cam is None else np.ascontiguousarray(cam, np.int32)
    m = m if mk is None else np.ascontiguousarray(mk, np.int32)
    n = len(b) - 1
    T0 = np.ascontiguousarray(prob["T_start"], float).reshape(-1, 16)
    opt = mpe.MpeBodyCalibrationOptions(scale, max_it, tol)
    outs = [np.full(17 * 3 * 8, sentinel, np.uint8), np.full(max(n, 1) * 16 * 8, sentinel, np.uint8),
            np.full(17 * 9 * 8, sentinel, np.uint8), np.full(max(n, 1) * 4, sentinel, np.uint8),
            np.full(C.sizeof(mpe.MpeBodyCalibrationReport), sentinel, np.uint8)]
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    arg = dict(cameras=cams, markers=xyz.ctypes.data_as(dp), view_begin=b.ctypes.data_as(ip), row_camera=c.ctypes.data_as(ip),
               row_marker=m.ctypes.data_as(ip), uv=uv.ctypes.data_as(dp), T0=T0.ctypes.data_as(dp), P=outs[0].ctypes.data_as(dp),
               report=C.cast(outs[4].ctypes.data, C.POINTER(mpe.MpeBodyCalibrationReport)))
    for k in null:
        arg[k] = None
    rc = lib.mpe_body_calibrate(hip._h, arg["cameras"], n_cameras, arg["markers"], n_markers, arg["view_begin"], arg["row_camera"],
                                arg["row_marker"], arg["uv"], n, arg["T0"], C.byref(opt), arg["P"], outs[1].ctypes.data_as(dp),
                                outs[2].ctypes.data_as(dp), outs[3].ctypes.data_as(ip), arg["report"])
    return rc, lib.mpe_last_error(hip._h).decode(), all(bool((o == sentinel).all()) for o in outs)


def test_refusals(hip):
    """Every refusal returns its code before any device work — mpe_last_error names it, no output is written — and the
    handle works afterwards: the same call as before the refusals gives the same bits."""
    ERR_ARG, ERR_UNSUPPORTED = -1, -3
    prob = wbb.random_body_calibration(np.random.default_rng(47), 3, 4, 4, p_missing=0.0)
    want = _calibrate(hip, prob)
    n_rows = sum(len(rows) for rows in prob["views"])
    assert n_rows == 48
    cases = [(dict(null=("cameras",)), ERR_ARG, "cameras"), (dict(null=("markers",)), ERR_ARG, "markers_xyz"),
             (dict(null=("view_begin",)), ERR_ARG, "view_begin"), (dict(null=("T0",)), ERR_ARG, "T_view_init"),
             (dict(null=("P",)), ERR_ARG, "markers_out"), (dict(null=("report",)), ERR_ARG, "report"),
             (dict(null=("row_camera",)), ERR_ARG, "row array"), (dict(null=("row_marker",)), ERR_ARG, "row array"),
             (dict(null=("uv",)), ERR_ARG, "row array"),
             (dict(n_cameras=0), ERR_ARG, "n_cameras"), (dict(n_cameras=17), ERR_ARG, "n_cameras"),
             (dict(n_markers=0), ERR_ARG, "n_markers"), (dict(n_markers=17), ERR_ARG, "n_markers"),
             (dict(cam=[0, 1, 3] + [0] * (n_rows - 3)), ERR_ARG, "camera index"),
             (dict(cam=[0, -1] + [0] * (n_rows - 2)), ERR_ARG, "camera index"),
             (dict(mk=[0, 1, 4] + [0] * (n_rows - 3)), ERR_ARG, "marker index"),
             (dict(mk=[0, -1] + [0] * (n_rows - 2)), ERR_ARG, "marker index"),
             (dict(begin=[0, 12, 6, 36, 48]), ERR_ARG, "view_begin"), (dict(begin=[-1, 12, 24, 36, 48]), ERR_ARG, "view_begin"),
             (dict(begin=[0, 257], cam=[k % 3 for k in range(257)], mk=[k % 4 for k in range(257)]), ERR_UNSUPPORTED, "rows"),
             (dict(scale=2), ERR_ARG, "scale"), (dict(scale=-2), ERR_ARG, "scale"),
             (dict(max_it=0), ERR_ARG, "max_iterations"), (dict(tol=0.0), ERR_ARG, "step_tolerance"),
             (dict(tol=float("nan")), ERR_ARG, "step_tolerance")]
    big = dict(prob)
    big["views"] = [[(k % 3, k % 4, np.zeros(2)) for k in range(257)]]
    for kw, code, word in cases:
        rc, msg, clean = _raw(hip, big if "rows" == word else prob, **kw)
        assert rc == code and word in msg and clean, (kw, rc, msg, clean)
    rc, msg, clean = _raw(hip, prob)                         # (the helper's call as such is a good one)
    assert rc == 1 and not clean
    assert _same(_calibrate(hip, prob), want)
    _refused_while_a_submission_is_pending(prob)


def _refused_while_a_submission_is_pending(prob):
    """A lock-step submission that is not collected yet owns the handle's staging memory and device buffers: a calibration
    in between is refused with MPE_ERR_ARG before it touches anything — every output keeps the sentinel, the submission
    collects the records it would have given alone, and the calibration afterwards gives the bits it gave before.  (The
    submission is tests/test_device_frame_streams.py's: one device frame, a whole-image item and a tracked one.)"""
    import torch
    lib = mpe.load_library()
    q = synth.make_sequence("C2", 1, seed=990)
    rows, cols = int(q["rows"]), int(q["cols"])
    d_img = torch.from_numpy(np.ascontiguousarray(q["frames"][0])).cuda()
    K, D = np.ascontiguousarray(q["K"], np.float64), np.ascontiguousarray(q["D"], np.float64)
    markers = np.ascontiguousarray(q["markers"], np.float64)
    P = mpe.demo_params()
    pred = np.ascontiguousarray(synth.project(q["T_true"][0], q["markers"], q["K"]), np.float64)
    px = synth.distort_px(pred, q["K"], q["D"])
    x0, y0 = [max(0, int(v) - 40) for v in px.min(0)]
    x1, y1 = min(cols, int(px[:, 0].max()) + 40), min(rows, int(px[:, 1].max()) + 40)
    su = (mpe.binding.TrackSetup * 1)(mpe.binding.TrackSetup(C.addressof(P), K.ctypes.data, D.ctypes.data, len(D),
                                                             markers.ctypes.data, len(markers)))
    it = (mpe.binding.TrackItem * 2)()
    it[0] = mpe.binding.TrackItem(d_img.data_ptr(), 0, 0, cols, rows, None)
    it[1] = mpe.binding.TrackItem(d_img.data_ptr(), x0, y0, x1 - x0, y1 - y0, pred.ctypes.data)
    h = mpe.Handle(0)
    torch.cuda.synchronize()

    def submit():
        return lib.mpe_track_step_batch_setups_device_submit(h._h, it, None, 2, rows, cols, cols, su, 1)

    def collect():
        dets, corr, res = np.zeros(2, mpe.DETECTIONS_DTYPE), np.zeros(2 * 32, np.uint32), np.zeros(2, mpe.RESULT_DTYPE)
        assert lib.mpe_track_step_batch_collect(h._h, C.c_void_p(dets.ctypes.data), C.c_void_p(corr.ctypes.data),
                                                C.c_void_p(res.ctypes.data)) == 0
        assert res["status"][1] == 0 and dets["n"][0] == 5
        return dets.tobytes() + corr.tobytes() + res.tobytes()

    try:
        want = _calibrate(h, prob)
        assert want["ok"]
        assert submit() == 0
        ref = collect()
        assert submit() == 0
        rc, msg, clean = _raw(h, prob)
        assert rc == -1 and "a submitted batch has not been collected yet" in msg and clean, (rc, msg, clean)
        assert collect() == ref
        assert _same(_calibrate(h, prob), want)
    finally:
        lib.mpe_track_step_batch_cancel(h._h)
        h.close()


def test_a_failing_case_leaves_the_outputs_as_the_inputs(hip):
    """The construction (tests/test_rig_calibration.py's): view 0's start pose puts marker 0 exactly into the focal plane
    of camera 0 (E = I, T = [I | (0, 0, -p_z)]: z = 0 without rounding), so its projection is inf / NaN and every sum it
    enters is non-finite — on the device and in the witness alike."""
    prob = wbb.random_body_calibration(np.random.default_rng(48), 2, 3, 4, p_missing=0.0)
    prob["cameras"][0] = (prob["cameras"][0][0], np.eye(4))
    assert prob["views"][0][0][:2] == (0, 0)
    prob["T_start"][0] = np.eye(4)
    prob["T_start"][0][2, 3] = -prob["markers"][0][2]
    w = wbb.body_calibrate(prob["cameras"], prob["views"], prob["markers"], prob["T_start"])
    assert not w["ok"] and w["report"]["status"] == 1
    got = _calibrate(hip, prob)
    assert not got["ok"] and got["report"]["status"] == 1
    assert got["report"]["views_used"] == 3 and got["report"]["marker_state"] == [1] * 4
    assert got["markers"].tobytes() == np.ascontiguousarray(prob["markers"]).tobytes()
    assert got["T_views"].tobytes() == np.ascontiguousarray(prob["T_start"]).tobytes()
    assert not got["cov"].any() and got["view_used"].all()
    good = wbb.random_body_calibration(np.random.default_rng(49), 2, 3, 4, p_missing=0.0)
    wbb.check_against_witness(_calibrate(hip, good), good, "the handle afterwards")


def _rig_cameras(n):
    """n cameras of C2's image size on a 12 cm base line, turned a few degrees towards each other; camera 0 is the rig
    frame (tests/test_rig_fusion.py's rig)."""
    K0, D0 = synth.camera_for(480, 752)
    cams, E = [], []
    for c in range(n):
        K = K0.copy()
        K[0, 0] *= 1.0 + 0.02 * c
        K[1, 1] *= 1.0 - 0.015 * c
        K[0, 2] += 3.0 * c
        cams.append((K, D0 * (1.0 - 0.1 * c)))
        T = np.eye(4)
        if c:
            T[:3, :3] = synth.rodrigues([0.1, 1.0, 0.05 * c], 0.04 * c * (-1) ** c)
            T[:3, 3] = [0.06 * c * (-1) ** c, 0.01 * c, 0.005 * c]
        E.append(T)
    return cams, np.array(E)


def test_rendered_sequence_through_the_calibrator(hip):
    """40 rendered frames of a 2-camera rig whose body's LEDs are about 3 mm away from where the trackers believe them,
    through BodyCalibrator.step, then solve(): the call succeeds and agrees with the witness over the same stored rows,
    the residual shrinks, and the calibrated shape is nearer the true one (after a rigid alignment) than the start's.  The
    before / after figures are printed (tools/body_calibration_numbers.py records them in profiles/body_calibration.jsonl);
    no ratio is asserted."""
    cams, E_true = _rig_cameras(2)
    nominal = np.asarray(synth.CONFIGS["C2"]["markers"], float)
    truth = nominal + np.random.default_rng(50).normal(size=nominal.shape) * 0.003 / np.sqrt(3)
    seq = synth.make_rig_sequence("C2", 40, 5, cams, E_true, ang_speed=1.2, true_markers=truth)
    assert np.array_equal(seq["markers"], nominal) and np.array_equal(seq["markers_true"], truth)
    Ph = mpe.demo_params()
    trackers = [mpe.Tracker(hip, seq["markers"], K, D, Ph) for K, D in cams]
    cal = mpe.BodyCalibrator(hip, trackers, E_true)
    n_upd = 0
    for k in range(40):
        rec, info, upd = cal.step([f[k] for f in seq["frames"]], [seq["times"][k]] * 2)
        n_upd += int(upd.sum())
    # (the precondition: the trackers follow the body although their markers are off — which costs them updates, 61 of
    #  80 here: at least half of the tracker-frames update, and below at least 20 views carry the calibration, each with
    #  up to 20 residuals against its 6 pose unknowns and the 15 shared ones)
    assert n_upd >= 40, n_upd
    out = cal.solve()
    rep = out["report"]
    before, after = wbb.shape_error(nominal, truth, False), wbb.shape_error(out["markers"], truth, False)
    figures = dict(what="rendered sequence, 2 cameras x 5 markers x 40 frames, markers 3 mm off", views_used=rep["views_used"],
                   rows_used=rep["rows_used"], iterations=rep["iterations"], rms_before_px=rep["rms_before"],
                   rms_after_px=rep["rms_after"], shape_error_before_m=before, shape_error_after_m=after)
    print("body calibration end to end:", json.dumps(figures))
    assert out["ok"] and rep["marker_state"] == [1] * 5 and rep["views_used"] >= 20 and rep["scale_held"] == 0
    assert rep["rms_after"] < rep["rms_before"]
    assert after < before, (before, after)
    prob = dict(cameras=[(t.K, E_true[c]) for c, t in enumerate(trackers)], views=cal.views, markers=out["start"]["markers"],
                T_start=out["start"]["T_views"])
    wbb.check_against_witness(out, prob, "end to end")
    cal.apply()
    assert all(np.array_equal(t.markers, out["markers"]) for t in trackers)
    for t in trackers:
        t.close()
