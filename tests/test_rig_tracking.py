"""A body tracked with the whole rig on the device (mpe_rig_track_batch / k_rig_track, mpe_rig_track_trackers,
Rig.track, Rig.step(partial=True)): the smallest shapes that can go wrong and drawn problems against the numpy witness
(tests/witness_rig_track.py) with its criteria and margins; one round is mpe_rig_optimise_pose_batch over the matched rows
bit for bit, two rounds are two chained single rounds; a record does not depend on its batch; the refusals write nothing;
a body that is half occluded for EVERY camera keeps its pose (the parent's Rig.step loses it); a bright distractor beside
a predicted LED."""
import ctypes as C

import numpy as np
import pytest

import rpg_monocular_pose_estimator_amd as mpe
from rpg_monocular_pose_estimator_amd import synth
import witness_rig_track as W

pytestmark = pytest.mark.gpu
INF = float("inf")


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def dev_track(hip, problem, **options):
    cameras, markers, dets, T_pred, tol_m, tol_a = problem
    rec, match, info = hip.rig_track_batch(cameras, markers, [dets], [T_pred], tol_m, tol_a, **options)
    return rec[0], match[0], info[0]


@pytest.fixture(scope="module")
def shapes():
    s, redraws = W.shapes()
    assert redraws <= 1
    return s


def test_shapes_against_the_witness(hip, shapes):
    for s in shapes:
        rec, match, info = dev_track(hip, s["problem"], **s["options"])
        w = W.check_against_witness(rec, match, info, s["problem"], s["options"], s["name"])
        W.check_expectation(s, w)


def test_drawn_problems_against_the_witness(hip):
    """120 drawn problems in ONE call per rig would need one rig; here every problem has its own rig, one call each."""
    rng = np.random.default_rng(404)
    redraws, kinds = 0, set()
    for k in range(120):
        kw = dict(n_cam=3, seen=[4, 3, 3], displace=(1, float(rng.uniform(4, 11)))) if k % 3 == 1 else {}
        options = dict(max_rounds=1 + k % 3)
        problem, _, w, r = W.draw(rng, options, **kw)
        redraws += r
        rec, match, info = dev_track(hip, problem, **options)
        W.check_against_witness(rec, match, info, problem, options, k)
        kinds.add((w["reason"], w["rounds"]))
    assert redraws <= 6 and {(0, 1), (0, 2), (4, 1)} <= kinds, (redraws, kinds)


def test_one_round_is_the_refinement_and_two_rounds_are_two_chained(hip, shapes):
    rng = np.random.default_rng(405)
    problems = [s["problem"] for s in shapes]
    for k in range(40):
        kw = dict(n_cam=3, seen=[4, 3, 3], displace=(1, float(rng.uniform(4, 11)))) if k % 2 else {}
        problems.append(W.random_problem(rng, **kw)[0])
    n_pose, kinds = 0, set()
    for k, problem in enumerate(problems):
        cameras, markers, dets, T_pred, tol_m, tol_a = problem
        inf = np.full(len(cameras), INF)
        rec, match, info = dev_track(hip, problem, max_rounds=1)
        if rec["status"] == 0:
            rows = W.rows_of(match.astype(np.int64), markers, dets)
            assert _same(hip.rig_optimise_pose_batch(cameras, [rows], [T_pred])[0], rec), k
            n_pose += 1
        # two rounds = a round that accepts anything, then a round from its pose with the accept tolerance for both
        two = dev_track(hip, problem, max_rounds=2)
        r1, m1, i1 = dev_track(hip, (cameras, markers, dets, T_pred, tol_m, inf), max_rounds=1)
        if r1["status"] != 0:
            want = (r1, m1, i1)
        else:
            want = dev_track(hip, (cameras, markers, dets, r1["T"].reshape(4, 4), tol_a, tol_a), max_rounds=1)
            if np.array_equal(want[1], m1):              # a stable row set: the first refinement stands
                want = (rec, match, info)
        assert np.array_equal(two[1], want[1]) and two[2]["reason"] == want[2]["reason"], k
        assert two[0]["status"] == want[0]["status"] and two[0]["gn_iterations"] == want[0]["gn_iterations"], k
        if two[0]["status"] == 0:
            assert _same(two[0]["T"], want[0]["T"]) and _same(two[0]["cov"], want[0]["cov"]), k
        else:
            assert np.array_equal(two[0]["T"].reshape(4, 4), np.asarray(T_pred, float)) and not two[0]["cov"].any(), k
        kinds.add((int(two[2]["reason"]), int(two[2]["rounds"])))
    # (the 20 undisturbed drawn problems and most shapes have a pose after one round; a displaced detection is reason 4 there)
    assert n_pose >= 25 and {(0, 1), (0, 2)} <= kinds, (n_pose, kinds)


def test_a_record_does_not_depend_on_its_batch(hip):
    """Calls of 1, 5 and 67 problems over one rig with the reasons 1 .. 4 between good problems: every record, match block
    and info record equals the problem submitted alone, bit for bit; the same run twice gives the same bits."""
    cameras, markers, tol_m, tol_a, options, items, kinds = W.mixed_batch(67)

    def call(sub):
        return hip.rig_track_batch(cameras, markers, [d for d, _ in sub], [T for _, T in sub], tol_m, tol_a, **options)

    alone = [call([it]) for it in items]
    assert [int(a[2]["reason"][0]) for a in alone] == kinds
    for a, k, (_, T) in zip(alone, kinds, items):
        assert (a[0]["status"][0] == 0) == (k == 0)
        if k:
            assert np.array_equal(a[0]["T"][0].reshape(4, 4), T) and not a[0]["cov"][0].any()
    for n in (1, 5, 67):
        rec, match, info = call(items[:n])
        for k in range(n):
            assert _same(rec[k], alone[k][0][0]) and _same(match[k], alone[k][1][0]) and _same(info[k], alone[k][2][0]), (n, k)
    again = call(items)
    assert _same(again[0], rec) and _same(again[1], match) and _same(again[2], info)


def _raw(hip, sentinel=0x5a, **kw):
    """mpe_rig_track_batch on a good two-camera problem with the named arguments replaced -> (rc, message, nothing written)"""
    lib = hip._lib
    cams = mpe.binding.pack_rig_cameras([W.exact_camera()] * 17)
    a = dict(h=hip._h, cams=cams, n_cam=2, mk=np.array(W.exact_problem("claimed_tie")[0][1]), n_mk=6,
             begin=np.array([0, 5, 10], np.int32), xy=np.tile(W.exact_problem("claimed_tie")[0][2][0], (14, 1)),
             tm=np.full(17, 12.0), ta=np.full(17, 6.0), n=1, T=np.tile(np.eye(4).reshape(16), (2, 1)),
             opt=mpe.MpeRigTrackOptions(2, 4, 3), info=True)
    a.update(kw)
    n = max(a["n"], 1)
    rec = np.full(n * mpe.RESULT_DTYPE.itemsize, sentinel, np.uint8)
    match = np.full(n * 17 * 16 * 4, sentinel, np.uint8)
    info = np.full(n * mpe.RIG_TRACK_INFO_DTYPE.itemsize, sentinel, np.uint8)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    ptr = lambda x, t: None if x is None else x.ctypes.data_as(t)  # noqa: E731
    rc = lib.mpe_rig_track_batch(a["h"], a["cams"], a["n_cam"], ptr(a["mk"], dp), a["n_mk"], ptr(a["begin"], ip), ptr(a["xy"], dp),
                                 ptr(a["tm"], dp), ptr(a["ta"], dp), a["n"], ptr(a["T"], dp),
                                 None if a["opt"] is None else C.byref(a["opt"]), rec.ctypes.data if a.get("out", True) else None,
                                 match.ctypes.data, info.ctypes.data if a["info"] else None)
    clean = bool((rec == sentinel).all() and (match == sentinel).all() and (info == sentinel).all())
    return rc, lib.mpe_last_error(hip._h).decode(), clean


def test_refusals_write_nothing(hip):
    ERR_ARG, ERR_UNSUPPORTED = -1, -3
    for null in ("cams", "mk", "begin", "tm", "ta", "T"):
        rc, msg, clean = _raw(hip, **{null: None})
        assert rc == ERR_ARG and "null" in msg and clean, null
    rc, msg, clean = _raw(hip, out=False)
    assert rc == ERR_ARG and clean
    for name, values, word in (("n_cam", (0, 17), "n_cameras"), ("n_mk", (0, 17), "n_markers")):
        for v in values:
            rc, msg, clean = _raw(hip, **{name: v})
            assert rc == ERR_ARG and word in msg and clean, (name, v)
    rc, msg, clean = _raw(hip, begin=np.array([0, 5, 4], np.int32))
    assert rc == ERR_ARG and "det_begin" in msg and clean
    rc, msg, clean = _raw(hip, begin=np.array([-1, 5, 10], np.int32))
    assert rc == ERR_ARG and "det_begin" in msg and clean
    rc, msg, clean = _raw(hip, begin=np.array([0, 65, 70], np.int32), xy=np.zeros((70, 2)))
    assert rc == ERR_UNSUPPORTED and "MPE_MAX_DETECTIONS" in msg and clean
    for opt in ((0, 4, 3), (5, 4, 3), (2, 2, 3), (2, 4, 0)):
        rc, msg, clean = _raw(hip, opt=mpe.MpeRigTrackOptions(*opt))
        assert rc == ERR_ARG and clean, opt
    for bad in (0.0, -1.0, float("nan")):
        for name in ("tm", "ta"):
            tol = np.full(17, 5.0)
            tol[1] = bad
            rc, msg, clean = _raw(hip, **{name: tol})
            assert rc == ERR_ARG and "tolerance" in msg and clean, (name, bad)
    rc, msg, clean = _raw(hip, n=0)                      # nothing to do, nothing submitted
    assert rc == 0 and clean
    # a lock-step submission that is not collected yet
    img = np.zeros((64, 64), np.uint8)
    P = mpe.demo_params()
    K, D, M = np.ascontiguousarray(W.exact_camera()[0]).reshape(9), np.zeros(5), np.ascontiguousarray(synth.M4, float)
    item = mpe.binding.TrackItem(img.ctypes.data, 0, 0, 64, 64, None)
    dp = C.POINTER(C.c_double)
    assert hip._lib.mpe_track_step_batch_submit(hip._h, C.byref(item), 1, 64, 64, C.c_size_t(64), C.byref(P), K.ctypes.data_as(dp),
                                                D.ctypes.data_as(dp), len(D), M.ctypes.data_as(dp), 4) == 0
    try:
        rc, msg, clean = _raw(hip)
        assert rc == ERR_ARG and "not been collected" in msg and clean
    finally:
        assert hip._lib.mpe_track_step_batch_cancel(hip._h) == 0
    # ... and the call as such is a good one: +inf tolerances, the default options, no info wanted
    rc, msg, clean = _raw(hip, tm=np.full(17, INF), opt=None, info=False)
    assert rc == 0 and not clean
    # mpe_rig_track_trackers refuses what mpe_rig_fuse_trackers refuses
    Kc, Dc = synth.camera_for(480, 752)
    other = mpe.Handle()
    try:
        t0, t1, t2 = mpe.Tracker(hip, synth.M5, Kc, Dc, P), mpe.Tracker(hip, synth.M4, Kc, Dc, P), mpe.Tracker(other, synth.M5, Kc, Dc, P)
        E = np.tile(np.eye(4), (2, 1, 1))
        for pair, word in (((t0, t1), "marker set"), ((t0, t2), "one handle"), ((t0, t0), "twice")):
            with pytest.raises(mpe.MpeError, match=word):
                mpe.Rig(hip, pair, E).track(np.eye(4))
        found, rec, match, info = mpe.Rig(hip, (t0,), E[:1]).track(np.eye(4))   # a tracker that has seen no frame: no row
        assert not found and rec["status"][0] == 1 and info["reason"][0] == 1 and not match.any()
        for t in (t0, t1, t2):
            t.close()
    finally:
        other.close()


def _run_scenario(hip, seq, cams, E, partial, **params):
    ts = [mpe.Tracker(hip, seq["markers"], K, D, mpe.demo_params(**params)) for K, D in cams]
    rig = mpe.Rig(hip, ts, E)
    out = []
    for k in range(len(seq["times"])):
        step = rig.step([f[k] for f in seq["frames"]], [seq["times"][k]] * len(ts), reseed=True, partial=partial)
        out.append(step + (rig.last_track, [t.image_points() for t in ts]))
    for t in ts:
        t.close()
    return out


def test_a_body_half_occluded_for_every_camera_keeps_its_pose(hip):
    """3 cameras, 14 frames; from frame 5 on camera 0 sees LEDs {0, 1, 2}, camera 1 {2, 3, 4} and camera 2 {0, 4}.  The
    parent's step (partial=False) has no rig pose on those frames; with partial=True they fuse with 8 rows from 3 cameras,
    reason 0, the translation within 5e-3 m of the truth (the bound tests/test_rig_fusion.py applies to fused poses).  The
    seed was chosen on the CPU (tests/test_rig_track_host.py, the oracle's detections through the host tier): 1.40 mm at
    the most on a partial frame, under half the bound."""
    seq, cams, E = W.scenario_sequence()
    S = W.SCENARIO
    plain = _run_scenario(hip, seq, cams, E, partial=False)
    whole = _run_scenario(hip, seq, cams, E, partial=True)
    worst = 0.0
    for k in range(S["frames"]):
        rec, info, upd, rr, fused, last, pts = whole[k]
        if k < S["full"]:
            assert plain[k][4] and fused and upd.all(), k  # (the precondition: every camera solves the full views)
            assert _same(rec, plain[k][0]) and np.array_equal(info, plain[k][1]) and np.array_equal(upd, plain[k][2]), k
            continue
        assert not plain[k][4] and not plain[k][2].any(), k  # the parent's behaviour: no camera, no rig pose
        assert [len(p) for p in pts] == [3, 3, 2], k
        assert fused and not upd.any() and last is not None, k
        track, match, tinfo = last
        assert _same(track, rr) and rr["status"][0] == 0 and rr["n_corr"][0] == 8 and rr["n_det"][0] == 3, k
        assert tinfo["reason"][0] == 0 and tinfo["rows"][0] == 8 and tinfo["distinct_markers"][0] == 5, k
        for c, ms in S["partial"].items():
            assert [m for m in range(5) if match[c, m]] == list(ms), (k, c)
        err = np.abs(rr["T"][0].reshape(4, 4) - seq["T_true"][k])[:3, 3].max()
        print("frame %d: %.3g m, residuals max %.3g rms %.3g px" % (k, err, tinfo["max_residual"][0], tinfo["rms"][0]))
        assert err < 5e-3, (k, err)
        worst = max(worst, err)
    print("largest translation error on a partial frame: %.3g m" % worst)


def test_a_bright_distractor_beside_a_predicted_led(hip):
    """The scenario's frame 8 with a spot as bright as an LED 9.5 px beside LED 1 in camera 0's image (nearer than some
    9 px the blob detection merges the two into one blob, or loses both to its shape filter), the trackers with a
    nearest-neighbour tolerance of 12 px: the distractor is a detection of its own within the match tolerance of the
    predicted LED.  Pinned: the LED's own detection is nearer to the prediction, the nearest-detection rule takes it in
    round 0 and the distractor gets no row — neither the second round nor the uniqueness rule is needed; the frame fuses
    with the same 8 rows in one round, reason 0, within the bound.  (On the CPU tier's simulation of this frame: the
    prediction 0.85 px from the LED's detection, 8.6 px from the distractor's, the pose 1.05 mm off.)"""
    seq, cams, E = W.scenario_sequence()
    S = W.SCENARIO
    k_hit = 8
    K, D, rows, cols = seq["cameras"][0]
    led = synth.distort_px(synth.project(E[0] @ seq["T_true"][k_hit], seq["markers"], K), K, D)[1]
    spot = synth.render_frame(np.random.default_rng(1), [led + np.array([9.5, 0.0])], rows, cols, synth.CONFIGS["C2"]["spot_sigma"],
                              bg_max=0)
    frames = [f.copy() for f in seq["frames"]]
    frames[0][k_hit] = np.maximum(frames[0][k_hit], spot)
    seq = dict(seq, frames=frames)
    out = _run_scenario(hip, seq, cams, E, partial=True, nearest_neighbour_pixel_tolerance=12.0)
    rec, info, upd, rr, fused, last, pts = out[k_hit]
    assert [len(p) for p in pts] == [4, 3, 2]            # the distractor is a detection of camera 0
    track, match, tinfo = last
    assert fused and _same(track, rr) and tinfo["reason"][0] == 0 and tinfo["rows"][0] == 8 and tinfo["rounds"][0] == 1
    assert [m for m in range(5) if match[0, m]] == list(S["partial"][0])
    d = np.sort(np.linalg.norm(pts[0] - pts[0][match[0, 1] - 1], axis=1))
    assert d[0] == 0.0 and 8.0 < d[1] < 11.0             # LED 1's row is its own detection, the distractor lies beside it
    uv = synth.project(E[0] @ mpe.predict_pose(out[k_hit - 1][3]["T"][0].reshape(4, 4), out[k_hit - 2][3]["T"][0].reshape(4, 4),
                                               seq["times"][k_hit - 1], seq["times"][k_hit - 2], seq["times"][k_hit]),
                       seq["markers"], K)[1]
    assert np.sort(np.linalg.norm(pts[0] - uv, axis=1))[1] < 12.0   # ... within the match tolerance of the predicted LED
    assert np.abs(rr["T"][0].reshape(4, 4) - seq["T_true"][k_hit])[:3, 3].max() < 5e-3
    for k in range(k_hit + 1, S["frames"]):              # ... and the frames behind it fuse as before
        assert out[k][4] and out[k][5][2]["rows"][0] == 8, k
