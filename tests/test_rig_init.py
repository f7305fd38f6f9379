"""A body found with the whole rig on the device (mpe_rig_init_batch / k_rig_init_*, mpe_rig_init_trackers, Rig.init,
Rig.step(init=True)): the exact shapes and drawn problems against the numpy witness (tests/witness_rig_init.py; its dicts
come from tests/golden/rig_init_witness.json, which the CPU tier holds against a fresh run); the tracking rounds behind the
winner are mpe_rig_track_batch from info.T_hyp bit for bit; a record does not depend on its batch; the refusals write
nothing; a body that NO camera sees four LEDs of from the first frame on gets its pose (the parent's Rig.step never has
one); a body that is lost is found again, and empty frames give no pose."""
import ctypes as C

import numpy as np
import pytest

import rpg_monocular_pose_estimator_amd as mpe
from rpg_monocular_pose_estimator_amd import synth
import witness_rig
import witness_rig_init as WI
import witness_rig_track as W

pytestmark = pytest.mark.gpu


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def dev_init(hip, problem, **options):
    cameras, markers, dets, tol_v, tol_a = problem
    rec, match, info = hip.rig_init_batch(cameras, markers, [dets], tol_v, tol_a, **options)
    return rec[0], match[0], info[0]


@pytest.fixture(scope="module")
def problems():
    """the exact shapes and every second drawn problem (30 with the body, 10 without), with the recorded witness dicts"""
    record = WI.recorded()
    shapes, _ = WI.shapes(record=record["shapes"])
    drawn, _ = WI.drawn_problems(record=record["drawn"])
    return shapes, drawn[::2]


def test_shapes_and_drawn_problems_against_the_witness(hip, problems):
    shapes, drawn = problems
    for s in shapes:
        rec, match, info = dev_init(hip, s["problem"], **s["options"])
        WI.check_against_witness(rec, match, info, s["problem"], s["options"], s["name"], w=s["w"])
        WI.check_expectation(s, s["w"])
    assert len(drawn) == 40
    reasons = set()
    for k, p in enumerate(drawn):
        rec, match, info = dev_init(hip, p["problem"])
        WI.check_against_witness(rec, match, info, p["problem"], None, k, w=p["w"])
        reasons.add(int(info["reason"]))
    assert {0, 1, 5} <= reasons, reasons


def test_a_list_of_64_detections(hip):
    """999 936 items in 7 812 blocks, the winner in the last one: known by construction (witness_rig_init.long_list)"""
    problem, expect = WI.long_list()
    rec, match, info = dev_init(hip, problem)
    WI.check_long_list(rec, match, info, expect)


def test_the_rounds_behind_the_winner_are_the_tracking_entrys(hip, problems):
    shapes, drawn = problems
    n = 0
    for p in [dict(s, options=s["options"]) for s in shapes] + [dict(p, options={}) for p in drawn]:
        cameras, markers, dets, tol_v, tol_a = p["problem"]
        rec, match, info = dev_init(hip, p["problem"], **p["options"])
        if int(info["reason"]) not in (0, 3, 4):
            continue
        o = dict(WI.DEFAULTS, **p["options"])
        r, m, i = hip.rig_track_batch(cameras, markers, [dets], [info["T_hyp"].reshape(4, 4)], tol_v, tol_a, max_rounds=o["max_rounds"],
                                      min_rows=o["min_rows"], min_markers=o["min_markers"])
        assert _same(m[0], match) and _same(i[0], info["track"]), p.get("name", p.get("kind"))
        assert int(i[0]["reason"]) == int(info["reason"])
        if rec["status"] == 0:
            assert _same(r[0], rec)
        n += 1
    assert n >= 25, n


def mixed_batch(n=33, seed=33):
    """n problems over ONE rig of three cameras and five markers with every way to end in turn: the body spread [3, 3, 2],
    [3, 2, 1], absent among clutter, [2, 2, 2] (no camera with three detections: reason 6), [4, 3, 0]"""
    rng = np.random.default_rng(seed)
    rig = (witness_rig.random_cameras(rng, 3), rng.uniform(-0.25, 0.25, (5, 3)))
    kinds = ([3, 3, 2], [3, 2, 1], None, [2, 2, 2], [4, 3, 0])
    items = []
    for k in range(n):
        seen = kinds[k % len(kinds)]
        problem, _ = WI.random_problem(rng, seen, clutter=0 if seen == [2, 2, 2] else 2, rig=rig)
        items.append(problem[2])
    return rig[0], rig[1], items


def test_a_record_does_not_depend_on_its_batch(hip):
    cameras, markers, items = mixed_batch()

    def call(sub):
        return hip.rig_init_batch(cameras, markers, sub, 3.0, 3.0)

    alone = [call([d]) for d in items]
    reasons = [int(a[2]["reason"][0]) for a in alone]
    assert {0, 1, 6} <= set(reasons), reasons
    for n in (1, 5, 33):
        rec, match, info = call(items[:n])
        for k in range(n):
            assert _same(rec[k], alone[k][0][0]) and _same(match[k], alone[k][1][0]) and _same(info[k], alone[k][2][0]), (n, k)
    again = call(items)
    assert _same(again[0], rec) and _same(again[1], match) and _same(again[2], info)


def _raw(hip, sentinel=0x5a, **kw):
    """mpe_rig_init_batch on a good two-camera problem with the named arguments replaced -> (rc, message, nothing written)"""
    lib = hip._lib
    cams = mpe.binding.pack_rig_cameras([W.exact_camera()] * 17)
    a = dict(h=hip._h, cams=cams, n_cam=2, mk=np.array(W.exact_problem("claimed_tie")[0][1]), n_mk=6,
             begin=np.array([0, 5, 10], np.int32), xy=np.tile(W.exact_problem("claimed_tie")[0][2][0], (14, 1)),
             tv=np.full(17, 12.0), ta=np.full(17, 6.0), n=1, opt=mpe.MpeRigInitOptions(2, 6, 4, 1), info=True)
    a.update(kw)
    n = max(a["n"], 1)
    rec = np.full(n * mpe.RESULT_DTYPE.itemsize, sentinel, np.uint8)
    match = np.full(n * 17 * 16 * 4, sentinel, np.uint8)
    info = np.full(n * mpe.RIG_INIT_INFO_DTYPE.itemsize, sentinel, np.uint8)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    ptr = lambda x, t: None if x is None else x.ctypes.data_as(t)  # noqa: E731
    rc = lib.mpe_rig_init_batch(a["h"], a["cams"], a["n_cam"], ptr(a["mk"], dp), a["n_mk"], ptr(a["begin"], ip), ptr(a["xy"], dp),
                                ptr(a["tv"], dp), ptr(a["ta"], dp), a["n"], None if a["opt"] is None else C.byref(a["opt"]),
                                rec.ctypes.data if a.get("out", True) else None, match.ctypes.data,
                                info.ctypes.data if a["info"] else None)
    clean = bool((rec == sentinel).all() and (match == sentinel).all() and (info == sentinel).all())
    return rc, lib.mpe_last_error(hip._h).decode(), clean


def test_refusals_write_nothing(hip):
    ERR_ARG, ERR_UNSUPPORTED = -1, -3
    before = hip.get_option("rig_init_submits")
    for null in ("cams", "mk", "begin", "tv", "ta"):
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
    # the item cap: a list of 64 with 6 markers is 41 664 x 120 = 5.0 M items; with 5 markers (2.5 M) it is admitted
    rc, msg, clean = _raw(hip, begin=np.array([0, 64, 64], np.int32), xy=np.zeros((64, 2)))
    assert rc == ERR_UNSUPPORTED and "2^22" in msg and clean
    for opt in ((0, 6, 4, 1), (5, 6, 4, 1), (2, 2, 4, 1), (2, 6, 0, 1), (2, 6, 4, -1)):
        rc, msg, clean = _raw(hip, opt=mpe.MpeRigInitOptions(*opt))
        assert rc == ERR_ARG and clean, opt
    for bad in (0.0, -1.0, float("nan")):
        for name in ("tv", "ta"):
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
    assert hip.get_option("rig_init_submits") == before  # no refusal reached the device
    # ... and the call as such is a good one: +inf tolerances, the default options, no info wanted
    rc, msg, clean = _raw(hip, tv=np.full(17, float("inf")), opt=None, info=False)
    assert rc == 0 and not clean and hip.get_option("rig_init_submits") == before + 1
    # mpe_rig_init_trackers refuses what mpe_rig_fuse_trackers refuses
    Kc, Dc = synth.camera_for(480, 752)
    other = mpe.Handle()
    try:
        t0, t1, t2 = mpe.Tracker(hip, synth.M5, Kc, Dc, P), mpe.Tracker(hip, synth.M4, Kc, Dc, P), mpe.Tracker(other, synth.M5, Kc, Dc, P)
        E = np.tile(np.eye(4), (2, 1, 1))
        for pair, word in (((t0, t1), "marker set"), ((t0, t2), "one handle"), ((t0, t0), "twice")):
            with pytest.raises(mpe.MpeError, match=word):
                mpe.Rig(hip, pair, E).init()
        found, rec, match, info = mpe.Rig(hip, (t0,), E[:1]).init()   # a tracker that has seen no frame: no item
        assert not found and rec["status"][0] == 1 and info["reason"][0] == 6 and info["n_items"][0] == 0 and not match.any()
        assert np.array_equal(rec["T"][0].reshape(4, 4), np.eye(4))
        for t in (t0, t1, t2):
            t.close()
    finally:
        other.close()


def _run(hip, seq, cams, E, init):
    ts = [mpe.Tracker(hip, seq["markers"], K, D, mpe.demo_params()) for K, D in cams]
    rig = mpe.Rig(hip, ts, E)
    out = []
    for k in range(len(seq["times"])):
        step = rig.step([f[k] for f in seq["frames"]], [seq["times"][k]] * len(ts), reseed=True, partial=True, init=init)
        out.append(step + (rig.last_track, rig.last_init, [len(t.image_points()) for t in ts]))
    for t in ts:
        t.close()
    return out


def test_a_body_no_camera_sees_four_leds_of_gets_its_pose(hip):
    """3 cameras, 10 frames; from frame 0 on camera 0 sees the LEDs {0, 1, 2}, camera 1 {2, 3, 4} and camera 2 {0, 4}.  The
    parent's Rig.step(partial=True, reseed=True) has no rig pose on any frame.  With init=True frame 0 gets its pose through
    the initialiser (reason 0, 8 rows, 3 cameras) in ONE submission, the later frames track from it, every translation
    within 5e-3 m of the truth (the bound tests/test_rig_fusion.py and test_rig_tracking.py apply).  The seed was chosen on
    the CPU (tests/test_rig_init_host.py, the oracle's detections through the host tier): 1.78 mm at the most."""
    seq, cams, E = WI.scenario_sequence()
    S = WI.SCENARIO
    plain = _run(hip, seq, cams, E, init=False)
    for k in range(S["frames"]):
        assert not plain[k][4] and not plain[k][2].any() and plain[k][6] is None, k   # the parent's behaviour: never a rig pose
    before = hip.get_option("rig_init_submits")
    found = _run(hip, seq, cams, E, init=True)
    assert hip.get_option("rig_init_submits") == before + 1
    worst = 0.0
    for k in range(S["frames"]):
        rec, info, upd, rr, fused, last_track, last_init, n_pts = found[k]
        assert n_pts == [3, 3, 2] and not upd.any() and fused and rr["status"][0] == 0, k
        if k == 0:
            irec, match, iinfo = last_init
            assert last_track is None and _same(irec, rr)
            assert iinfo["reason"][0] == 0 and iinfo["best_rows"][0] == 8 and iinfo["track"]["rows"][0] == 8, iinfo
        else:
            assert last_init is None and last_track is not None, k
            trec, match, tinfo = last_track
            assert _same(trec, rr) and tinfo["reason"][0] == 0 and tinfo["rows"][0] == 8, (k, tinfo)
        assert rr["n_corr"][0] == 8 and rr["n_det"][0] == 3, k
        for c, ms in S["partial"].items():
            assert [m for m in range(5) if match[c, m]] == list(ms), (k, c)
        err = np.abs(rr["T"][0].reshape(4, 4) - seq["T_true"][k])[:3, 3].max()
        print("frame %d: %.3g m" % (k, err))
        assert err < 5e-3, (k, err)
        worst = max(worst, err)
    print("largest translation error: %.3g m" % worst)


def test_a_lost_body_is_found_again(hip):
    """The same sequence with the frames 4 and 5 blank for every camera, init=True on every step: the blank frames give no
    pose (the tracking step, the fusion and the initialiser all say so), frame 6 is found by the initialiser again and the
    frames behind it track."""
    seq, cams, E = WI.scenario_sequence(blank=(4, 5))
    out = _run(hip, seq, cams, E, init=True)
    for k in range(WI.SCENARIO["frames"]):
        rec, info, upd, rr, fused, last_track, last_init, n_pts = out[k]
        if k in (4, 5):
            assert not fused and rr["status"][0] != 0 and last_init is not None and last_init[2]["reason"][0] != 0, (k, n_pts)
            continue
        assert fused and rr["status"][0] == 0 and rr["n_corr"][0] == 8, k
        assert (last_init is not None) == (k in (0, 6)), k
        if last_init is not None:
            assert last_init[2]["reason"][0] == 0 and last_init[2]["best_rows"][0] == 8, k
        assert np.abs(rr["T"][0].reshape(4, 4) - seq["T_true"][k])[:3, 3].max() < 5e-3, k
