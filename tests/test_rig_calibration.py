"""The extrinsics of a rig calibrated from the body it tracks, on the device (mpe_rig_calibrate: the k_rig_ba_* kernels,
Handle.rig_calibrate, RigCalibrator), at the smallest shapes at which the kernels can still go wrong, against the numpy
witness (tests/witness_rig_ba.py) with its criteria: extrinsics and view poses within 1e-9, covariance
allclose(rtol=1e-5, atol=1e-12), iterations within +-1, states / counts / flags equal."""
import ctypes as C

import numpy as np
import pytest

import rpg_monocular_pose_estimator_amd as mpe
from rpg_monocular_pose_estimator_amd import synth
import witness_rig_ba as wba

pytestmark = pytest.mark.gpu


def _calibrate(hip, prob, **kw):
    return hip.rig_calibrate(prob["cameras"], prob["views"], prob["T_start"], **kw)


def _same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("T_cam_rig", "T_views", "cov", "view_used")) \
        and a["report"] == b["report"] and a["ok"] == b["ok"]


def test_two_cameras_two_views(hip):
    prob = wba.random_calibration(np.random.default_rng(41), 2, 2, n_markers=4, seen=(4, 4), p_missing=0.0)
    got = _calibrate(hip, prob)
    assert got["ok"] and got["report"]["views_used"] == 2 and got["report"]["rows_used"] == 16
    w = wba.check_against_witness(got, prob, "2 x 2 x 4")
    assert w["report"]["iterations"] <= 10
    assert got["report"]["rms_after"] <= got["report"]["rms_before"]


def test_sixteen_cameras_of_sixteen_markers(hip):
    """256 rows a view and a 90 x 90 reduced system: the caps of both."""
    prob = wba.random_calibration(np.random.default_rng(42), 16, 3, n_markers=16, seen=(16, 16), p_missing=0.0)
    assert all(len(rows) == 256 for rows in prob["views"])
    got = _calibrate(hip, prob)
    assert got["ok"] and got["report"]["camera_state"] == [0] + [1] * 15 and got["report"]["rows_used"] == 768
    w = wba.check_against_witness(got, prob, "16 x 16 x 3")
    assert w["report"]["iterations"] <= 10


@pytest.mark.parametrize("n_views,n_used", [(65, 56), (84, 68), (300, 233)])
def test_view_counts_across_wave_block_and_chunk_boundaries(hip, n_views, n_used):
    """3 cameras of 4 markers, cameras missing at random (so views of one camera or none are among them): 65 views, of
    which 56 are used — fewer than a wave has lanes —, 84 with 68 used — four more than the 64 views of an update block
    and of a staging pass of the reduction —, and 300 with 233 used (four of each, the last partial); then the same call
    with the records of only a few views on the device at a time (chunks of 9 or 10 views, the last one shorter): the
    same bits."""
    prob = wba.random_calibration(np.random.default_rng(43 + n_views), 3, n_views, n_markers=4, seen=(4, 4), p_missing=0.3)
    got = _calibrate(hip, prob)
    assert got["ok"] and got["report"]["views_used"] == n_used
    wba.check_against_witness(got, prob, n_views)
    hip.set_option("rig_ba_record_kb", 16)
    try:
        assert hip.get_option("rig_ba_record_kb") == 16
        chunked = _calibrate(hip, prob)
    finally:
        hip.set_option("rig_ba_record_kb", 0)
    assert _same(chunked, got)


def test_held_cameras_and_unused_views(hip):
    """A view of one camera, a view of 2 rows, a camera without rows and a camera that shares no view with the others:
    the reported states and counts are the witness's, and what is not calibrated comes back as it went in, bit for bit."""
    prob = wba.random_calibration(np.random.default_rng(44), 5, 14, n_markers=4, seen=(4, 4), p_missing=0.0)
    views = []
    for f, rows in enumerate(prob["views"]):
        rows = [r for r in rows if r[0] != 2]                                    # camera 2 brings no row
        views.append([r for r in rows if r[0] != 4])
        views.append([r for r in rows if r[0] == 4])                             # camera 4 only ever alone
    views[6] = [r for r in views[6] if r[0] == 1]                                # a view of one camera
    views[10] = views[10][:1] + views[10][-1:]                                   # a view of 2 rows (cameras 0 and 3)
    prob["views"] = views
    prob["T_start"] = np.repeat(prob["T_start"], 2, axis=0)
    got = _calibrate(hip, prob)
    assert got["ok"] and got["report"]["camera_state"] == [0, 1, 2, 1, 2]
    assert list(got["view_used"]) == [f % 2 == 0 and f not in (6, 10) for f in range(28)]
    assert got["report"]["views_used"] == 12 and got["report"]["camera_rows"][2] == 0 and got["report"]["camera_rows"][4] == 0
    wba.check_against_witness(got, prob, "held and unused")
    for c in (0, 2, 4):
        assert got["T_cam_rig"][c].tobytes() == np.ascontiguousarray(prob["cameras"][c][1]).tobytes(), c
        assert not got["cov"][c].any(), c
    unused = ~got["view_used"]
    assert got["T_views"][unused].tobytes() == np.ascontiguousarray(prob["T_start"][unused]).tobytes()
    # the reference camera without a row: nothing is calibrated, everything comes back
    prob["views"] = [[r for r in rows if r[0] != 0] for rows in views]
    got = _calibrate(hip, prob)
    assert not got["ok"] and got["report"]["status"] == 1 and got["report"]["views_used"] == 0
    assert got["report"]["camera_state"] == [0, 2, 2, 2, 2] and not got["view_used"].any()
    assert got["T_views"].tobytes() == np.ascontiguousarray(prob["T_start"]).tobytes()
    assert got["T_cam_rig"].tobytes() == np.ascontiguousarray([E for _, E in prob["cameras"]]).tobytes()
    wba.check_against_witness(got, prob, "no reference rows")


def test_the_same_call_twice_gives_the_same_bits(hip):
    prob = wba.random_calibration(np.random.default_rng(45), 4, 70, p_missing=0.3)
    first = _calibrate(hip, prob, reference_camera=1)
    hip.rig_optimise_pose_batch(prob["cameras"], [prob["views"][0]], [prob["T_start"][0]])   # (another user of the buffers)
    second = _calibrate(hip, prob, reference_camera=1)
    assert first["ok"] and first["report"]["camera_state"][1] == 0 and _same(first, second)
    wba.check_against_witness(first, prob, "reference camera 1", reference_camera=1)


def _raw(hip, prob, n_cameras=None, begin=None, cam=None, ref=0, max_it=50, tol=1e-10, null=(), sentinel=0x5a):
    """mpe_rig_calibrate through ctypes with one argument spoilt -> (rc, message, every output still the sentinel)"""
    lib = hip._lib
    cams, b, c, xyz, uv = mpe.binding.pack_rig_views(prob["cameras"] + [prob["cameras"][0]] * 16, prob["views"])
    n_cameras = len(prob["cameras"]) if n_cameras is None else n_cameras
    b = b if begin is None else np.ascontiguousarray(begin, np.int32)
    c = c if cam is None else np.ascontiguousarray(cam, np.int32)
    n = len(b) - 1
    T0 = np.ascontiguousarray(prob["T_start"], float).reshape(-1, 16)
    opt = mpe.MpeRigCalibrationOptions(ref, max_it, tol)
    outs = [np.full(17 * 16 * 8, sentinel, np.uint8), np.full(max(n, 1) * 16 * 8, sentinel, np.uint8),
            np.full(17 * 36 * 8, sentinel, np.uint8), np.full(max(n, 1) * 4, sentinel, np.uint8),
            np.full(C.sizeof(mpe.MpeRigCalibrationReport), sentinel, np.uint8)]
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    arg = dict(cameras=cams, view_begin=b.ctypes.data_as(ip), row_camera=c.ctypes.data_as(ip), xyz=xyz.ctypes.data_as(dp),
               uv=uv.ctypes.data_as(dp), T0=T0.ctypes.data_as(dp), E=outs[0].ctypes.data_as(dp), report=C.cast(outs[4].ctypes.data, C.POINTER(mpe.MpeRigCalibrationReport)))
    for k in null:
        arg[k] = None
    rc = lib.mpe_rig_calibrate(hip._h, arg["cameras"], n_cameras, arg["view_begin"], arg["row_camera"], arg["xyz"], arg["uv"], n,
                               arg["T0"], C.byref(opt), arg["E"], outs[1].ctypes.data_as(dp), outs[2].ctypes.data_as(dp),
                               outs[3].ctypes.data_as(ip), arg["report"])
    return rc, lib.mpe_last_error(hip._h).decode(), all(bool((o == sentinel).all()) for o in outs)


def test_refusals(hip):
    """Every refusal returns its code before any device work — mpe_last_error names it, no output is written — and the
    handle works afterwards: the same call as before the refusals gives the same bits."""
    ERR_ARG, ERR_UNSUPPORTED = -1, -3
    prob = wba.random_calibration(np.random.default_rng(46), 3, 4, n_markers=4, seen=(4, 4), p_missing=0.0)
    want = _calibrate(hip, prob)
    n_rows = sum(len(rows) for rows in prob["views"])
    cases = [(dict(null=("cameras",)), ERR_ARG, "cameras"), (dict(null=("view_begin",)), ERR_ARG, "view_begin"),
             (dict(null=("T0",)), ERR_ARG, "T_view_init"), (dict(null=("E",)), ERR_ARG, "T_cam_rig_out"),
             (dict(null=("report",)), ERR_ARG, "report"), (dict(null=("row_camera",)), ERR_ARG, "row array"),
             (dict(null=("uv",)), ERR_ARG, "row array"), (dict(null=("xyz",)), ERR_ARG, "row array"),
             (dict(n_cameras=0), ERR_ARG, "n_cameras"), (dict(n_cameras=17), ERR_ARG, "n_cameras"),
             (dict(cam=[0, 1, 3] + [0] * (n_rows - 3)), ERR_ARG, "camera index"),
             (dict(cam=[0, -1] + [0] * (n_rows - 2)), ERR_ARG, "camera index"),
             (dict(begin=[0, 12, 6, 36, 48]), ERR_ARG, "view_begin"), (dict(begin=[-1, 12, 24, 36, 48]), ERR_ARG, "view_begin"),
             (dict(begin=[0, 257], cam=[k % 3 for k in range(257)]), ERR_UNSUPPORTED, "rows"),
             (dict(ref=3), ERR_ARG, "reference_camera"), (dict(ref=-1), ERR_ARG, "reference_camera"),
             (dict(max_it=0), ERR_ARG, "max_iterations"), (dict(tol=0.0), ERR_ARG, "step_tolerance"),
             (dict(tol=float("nan")), ERR_ARG, "step_tolerance")]
    big = dict(prob)
    big["views"] = [[(k % 3, np.zeros(3), np.zeros(2)) for k in range(257)]]
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
    """The construction: view 0's start pose puts marker 0 exactly into the focal plane of the reference camera (E = I,
    T = [I | (0, 0, -p_z)]: z = 0 without rounding), so its projection is inf / NaN and every sum it enters is non-finite
    — on the device and in the witness alike.  (Two cameras that see the same two markers in every view were tried first:
    the view poses are rank deficient there, but rounding keeps the pivots away from zero, and both the witness and the
    host build of the steps mostly wander for 50 iterations and end finite: that construction does not fail.)"""
    prob = wba.random_calibration(np.random.default_rng(47), 2, 3, n_markers=4, seen=(4, 4), p_missing=0.0)
    prob["cameras"][0] = (prob["cameras"][0][0], np.eye(4))
    p0 = prob["views"][0][0][1]
    assert prob["views"][0][0][0] == 0
    prob["T_start"][0] = np.eye(4)
    prob["T_start"][0][2, 3] = -p0[2]
    w = wba.rig_calibrate(prob["cameras"], prob["views"], prob["T_start"])
    assert not w["ok"] and w["report"]["status"] == 1
    got = _calibrate(hip, prob)
    assert not got["ok"] and got["report"]["status"] == 1
    assert got["report"]["views_used"] == 3 and got["report"]["camera_state"] == [0, 1]
    assert got["T_cam_rig"].tobytes() == np.ascontiguousarray([E for _, E in prob["cameras"]]).tobytes()
    assert got["T_views"].tobytes() == np.ascontiguousarray(prob["T_start"]).tobytes()
    assert not got["cov"].any() and got["view_used"].all()
    good = wba.random_calibration(np.random.default_rng(48), 2, 3, n_markers=4, seen=(4, 4), p_missing=0.0)
    wba.check_against_witness(_calibrate(hip, good), good, "the handle afterwards")


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


def _angle(R):
    return float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))


def test_rendered_sequence_through_the_calibrator(hip):
    """40 rendered frames of a 3-camera rig through RigCalibrator.step, then solve(): the residual does not grow, every
    calibrated extrinsic is closer to the truth than the start helper's in rotation angle and in translation, and the
    witness over the same stored rows gives the device's result within the criteria."""
    cams, E_true = _rig_cameras(3)
    seq = synth.make_rig_sequence("C2", 40, 5, cams, E_true, ang_speed=1.2)
    Ph = mpe.demo_params()
    trackers = [mpe.Tracker(hip, seq["markers"], K, D, Ph) for K, D in cams]
    cal = mpe.RigCalibrator(hip, trackers)
    n_upd = 0
    for k in range(40):
        rec, info, upd = cal.step([f[k] for f in seq["frames"]], [seq["times"][k]] * 3)
        n_upd += int(upd.sum())
    assert n_upd >= 3 * 36                                # (the precondition: the trackers follow the body)
    out = cal.solve()
    rep = out["report"]
    print("rig calibration end to end:", rep)
    assert out["ok"] and rep["camera_state"] == [0, 1, 1] and rep["views_used"] >= 36
    assert rep["rms_after"] <= rep["rms_before"]
    for c in (1, 2):
        for name, E in (("start", out["start"]["T_cam_rig"][c]), ("calibrated", out["T_cam_rig"][c])):
            d = E @ np.linalg.inv(E_true[c])
            print("camera %d %s: %.3e rad, %.3e m" % (c, name, _angle(d[:3, :3]), np.linalg.norm(E[:3, 3] - E_true[c][:3, 3])))
    for c in (1, 2):
        E0, E1 = out["start"]["T_cam_rig"][c], out["T_cam_rig"][c]
        assert _angle((E1 @ np.linalg.inv(E_true[c]))[:3, :3]) < _angle((E0 @ np.linalg.inv(E_true[c]))[:3, :3]), c
        assert np.linalg.norm(E1[:3, 3] - E_true[c][:3, 3]) < np.linalg.norm(E0[:3, 3] - E_true[c][:3, 3]), c
    prob = dict(cameras=[(t.K, out["start"]["T_cam_rig"][c]) for c, t in enumerate(trackers)], views=cal.views,
                T_start=out["start"]["T_views"])
    wba.check_against_witness(out, prob, "end to end")
    rig = cal.rig()
    assert np.array_equal(rig.T_cam_rig.reshape(3, 4, 4), out["T_cam_rig"])
    for t in trackers:
        t.close()
