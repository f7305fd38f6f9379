"""GPU tests of the wide tracked path — a stream whose ROI (or start-up frame) carries 65 .. 256 detections:
mpe_track_step_batch_wide (the lock-step time step with wide records), mpe_tracker_set_wide_frames (the state machine
behind every tracker entry) — against the narrow entries up to 64 detections and against the CPU oracle, whose
find_leds, Tracker and brute force take any count.  The oracle's passes are the cost of the module (about 15 s of CPU,
side by side on threads); every GPU body is milliseconds."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from rpg_monocular_pose_estimator_amd import synth
import rpg_monocular_pose_estimator_amd as mpe
from util import pose_diff, POS_TOL_M, ROT_TOL_RAD
from test_wide_frames import grid_frame, pose_scene, GRID_ROWS, GRID_COLS

pytestmark = pytest.mark.gpu

M4 = synth.M4
BORDER = 45
N_SEQ = 6
GLARE_COUNTS = {3: 107, 4: 130}    # detections in the frame-3 ROI of the two glare sequences (by the oracle)
KEYS = ("updated", "roi", "it_since_initialized", "n_det", "n_corr", "used_bruteforce")


def paint(img, box, leds, keep, limit=None):
    """4 x 5 rectangles of value 220 on a 12 x 11 pixel pitch, every cell 3 px inside `box` (x, y, w, h); cells whose
    centre is within `keep` px of a point of `leds` are skipped; at most `limit` rectangles.  -> their number."""
    x0, y0, w, h = box
    n = 0
    for y in range(y0 + 3, y0 + h - 3 - 11 + 1, 11):
        for x in range(x0 + 3, x0 + w - 3 - 12 + 1, 12):
            if np.linalg.norm(leds - np.array([x + 2.0, y + 1.5]), axis=1).min() <= keep:
                continue
            if limit is not None and n >= limit:
                return n
            img[y:y + 4, x:x + 5] = 220
            n += 1
    return n


def _leds(d, T):
    return synth.distort_px(synth.project(T, d["markers"], d["K"]), d["K"], d["D"])


def _oracle_run(orc, d, frames, times, **kw):
    to = orc.Tracker(d["markers"], d["K"], d["D"], orc.make_params(**kw))
    out = [to.estimate(frames[k], times[k]) for k in range(len(frames))]
    to.close()
    return out


def _build(orc):
    """The sequences of the module (name -> dict(d, frames, times, kw, glare frame)), their oracle records, and the clean
    run of seeds 3 / 4 (its ROIs place the rectangles: the ROI of frame 3 depends on frames 0 .. 2 alone)."""
    seq, base = {}, {}
    for seed in (3, 4):
        d = synth.make_sequence("C1", N_SEQ, seed)
        base[seed] = dict(d=d, rec=_oracle_run(orc, d, d["frames"], d["times"], roi_border_thickness=BORDER))
        f = d["frames"].copy()
        paint(f[3], base[seed]["rec"][3]["roi"], _leds(d, d["T_true"][3]), 14.0)
        seq["a%d" % seed] = dict(d=d, frames=f, times=d["times"], kw=dict(roi_border_thickness=BORDER), glare=3)
    d = base[3]["d"]
    # (b) the body jumps 0.03 m in x on frame 3, into 64 rectangles
    T = d["T_true"][3].copy()
    T[0, 3] += 0.03
    f = d["frames"].copy()
    f[3] = synth.render_frame(np.random.default_rng([3, 3, 3]), _leds(d, T), d["rows"], d["cols"], synth.CONFIGS["C1"]["spot_sigma"])
    assert paint(f[3], base[3]["rec"][3]["roi"], np.vstack([_leds(d, d["T_true"][3]), _leds(d, T)]), 14.0, limit=64) == 64
    seq["b"] = dict(d=d, frames=f, times=d["times"], kw=dict(roi_border_thickness=BORDER), glare=3)
    # (c) 66 rectangles in the start-up frame
    f = d["frames"].copy()
    assert paint(f[0], (197, 57, 406, 336), _leds(d, d["T_true"][0]), 40.0, limit=66) == 66
    seq["c"] = dict(d=d, frames=f, times=d["times"], kw=dict(roi_border_thickness=BORDER), glare=0)
    # (d) one 1920 x 1200 frame of 70 spots, a real 5-marker pose among them, shown three times
    K, D = synth.camera_for(1200, 1920)
    rng = np.random.default_rng(70130)
    _, spots = pose_scene(rng, synth.M5, 70, K, D, 1200, 1920, 30.0, 60.0, False)
    fr = synth.render_frame(rng, spots, 1200, 1920, spot_sigma=3.0)
    seq["d"] = dict(d=dict(markers=synth.M5, K=K, D=D, rows=1200, cols=1920), frames=np.stack([fr, fr, fr]),
                    times=np.array([0.0, 0.02, 0.04]), kw=dict(back_projection_pixel_tolerance=0.3), glare=0)
    with ThreadPoolExecutor(len(seq)) as ex:   # (the oracle's C entries release the interpreter lock)
        recs = list(ex.map(lambda s: _oracle_run(orc, s["d"], s["frames"], s["times"], **s["kw"]), seq.values()))
    for s, r in zip(seq.values(), recs):
        s["ref"] = r
    return seq, base


@pytest.fixture(scope="module")
def scenes(orc):
    seq, base = _build(orc)
    # what the oracle did, as the issue records it
    for seed in (3, 4):
        r = seq["a%d" % seed]["ref"]
        assert r[3]["n_det"] == GLARE_COUNTS[seed] and r[3]["updated"] and not r[3]["used_bruteforce"] and r[3]["n_corr"] == 4
        assert all(x["updated"] and not x["used_bruteforce"] for x in r[4:])
    r = seq["b"]["ref"]
    assert r[3]["n_det"] == 68 and not r[3]["updated"] and r[3]["used_bruteforce"] and r[4]["updated"]
    r = seq["c"]["ref"]
    assert r[0]["n_det"] == 70 and not r[0]["updated"] and r[0]["used_bruteforce"] and r[1]["updated"] and r[1]["used_bruteforce"]
    r = seq["d"]["ref"]
    assert r[0]["n_det"] == 70 and r[0]["updated"] and r[0]["n_corr"] == 4 and r[1]["roi"] == (721, 665, 173, 246) and r[1]["n_det"] == 6
    return dict(seq=seq, base=base)


def _params(kw):
    return mpe.demo_params(**kw)


# ---- 1. the wide entry is the narrow entry up to 64 detections ---------------------------------------------------------

def _bgr(frames):
    return np.ascontiguousarray(np.repeat(np.asarray(frames)[..., None], 3, axis=-1))


@pytest.mark.parametrize("source", ["host", "device", "bgr8"])
def test_wide_entry_equals_narrow_entry_up_to_64(hip, scenes, source):
    """Frames 1 .. 5 of the two clean sequences in the oracle tracker's ROIs with the true poses' projections as
    predictions, plus two detection-only items, over two set-ups (the second lists the markers in reverse and has another
    nearest-neighbour tolerance): n, status and the coordinates of every detection, the rows and every byte of the result
    equal what mpe_track_step_batch_setups / _device / _device_encoded return."""
    imgs, rois, preds, which = [], [], [], []
    Mr = np.ascontiguousarray(M4[::-1])
    for seed in (3, 4):
        b = scenes["base"][seed]
        d = b["d"]
        for k in range(1, 6):
            s = (k + seed) % 2
            imgs.append(d["frames"][k])
            rois.append(b["rec"][k]["roi"])
            preds.append(synth.project(d["T_true"][k], Mr if s else M4, d["K"]))
            which.append(s)
    d = scenes["base"][3]["d"]
    for s, roi in ((0, (0, 0, d["cols"], d["rows"])), (1, scenes["base"][4]["rec"][2]["roi"])):
        imgs.append(scenes["base"][4]["d"]["frames"][2])
        rois.append(roi)
        preds.append(None)
        which.append(s)
    setups = [(M4, d["K"], d["D"], _params(dict(roi_border_thickness=BORDER))),
              (Mr, d["K"], d["D"], _params(dict(roi_border_thickness=BORDER, nearest_neighbour_pixel_tolerance=6.0)))]
    before = hip.get_option("wide_track_submits")
    if source == "host":
        narrow = hip.track_step_batch(imgs, rois, preds, setups, which)
        wide = hip.track_step_batch_wide(imgs, rois, preds, setups, which)
    else:
        import torch
        enc = "mono8" if source == "device" else "bgr8"
        dev = [torch.from_numpy(f if enc == "mono8" else _bgr(f)).cuda() for f in imgs]
        narrow = hip.track_step_batch_device(dev, rois, preds, setups, which, encoding=enc)
        wide = hip.track_step_batch_wide(dev, rois, preds, setups, which, encoding=enc)
    assert hip.get_option("wide_track_submits") == before + 1
    (nd, nc, nr), (wd, wc, wr) = narrow, wide
    assert (nr["status"][:10] == 0).all() and (nd["n"][:10] == 4).all(), (nr["status"], nd["n"])   # (poses were compared)
    assert (nr["status"][10:] == 1).all() and (nd["n"][10:] == 4).all()
    for i in range(len(imgs)):
        n = int(nd["n"][i])
        assert wd["n"][i] == n and wd["status"][i] == nd["status"][i], i
        assert wd["undist_xy"][i][:2 * n].tobytes() == nd["undist_xy"][i][:2 * n].tobytes(), i
        assert wd["dist_xy"][i][:2 * n].tobytes() == nd["dist_xy"][i][:2 * n].tobytes(), i
        assert np.array_equal(wc[i], nc[i]), (i, wc[i], nc[i])
        assert wr[i].tobytes() == nr[i].tobytes(), (i, wr[i], nr[i])


# ---- 2. ROI glare, stage level ----------------------------------------------------------------------------------------

def _first_strict_minimum_rows(pred, det, tol):
    rows = []
    for i, p in enumerate(np.asarray(pred, float)):
        du, dv = p[0] - det[:, 0], p[1] - det[:, 1]
        d2 = du * du + dv * dv
        best, bj = np.inf, 0
        for j in range(len(det)):
            if d2[j] < best:
                best, bj = d2[j], j + 1
        if np.sqrt(best) <= tol:
            rows.append((i + 1, bj))
    return np.array(rows, np.uint32).reshape(-1, 2)


def test_roi_glare_stage_level(hip, orc, scenes):
    """Frame 3 of the two glare sequences in the oracle's ROI, the true pose's projections as predictions: the 107 / 130
    detections bit-equal to the oracle's find_leds in that ROI, the rows those of the first strict minimum, status 0
    with 4 rows, pose and covariance those of the oracle's checkCorrespondences + optimisePose on these rows."""
    imgs, rois, preds = [], [], []
    for seed in (3, 4):
        s = scenes["seq"]["a%d" % seed]
        imgs.append(s["frames"][3])
        rois.append(s["ref"][3]["roi"])
        preds.append(synth.project(s["d"]["T_true"][3], M4, s["d"]["K"]))
    d = scenes["seq"]["a3"]["d"]
    P, Po = _params(dict(roi_border_thickness=BORDER)), orc.make_params(roi_border_thickness=BORDER)
    dets, corr, res = hip.track_step_batch_wide(imgs, rois, preds, [(M4, d["K"], d["D"], P)], None)
    for i, seed in enumerate((3, 4)):
        und, dist = orc.find_leds(imgs[i], Po, d["K"], d["D"], roi=rois[i])
        n = len(und)
        assert n == GLARE_COUNTS[seed] and dets["n"][i] == n and dets["status"][i] == 0, (seed, n, dets["n"][i], dets["status"][i])
        assert np.array_equal(dets["undist_xy"][i][:2 * n].reshape(-1, 2), und), seed
        assert np.array_equal(dets["dist_xy"][i][:2 * n].reshape(-1, 2), dist), seed
        rows = _first_strict_minimum_rows(preds[i], und, P.nearest_neighbour_pixel_tolerance)
        assert res["status"][i] == 0 and res["n_corr"][i] == 4 and res["n_det"][i] == n, (seed, res["status"][i], res["n_corr"][i])
        assert np.array_equal(corr[i][:4], rows) and not corr[i][4:].any(), (seed, corr[i][:4], rows)
        assert rows[:, 1].max() > mpe.MAX_MARKERS    # (indices beyond the compact record's)
        ok, T0 = orc.check_correspondences(und, M4, d["K"], Po, rows)
        assert ok
        T, cov, _ = orc.optimise_pose(und, M4, d["K"], rows, T0)
        dp, dr = pose_diff(res["T"][i].reshape(4, 4), T)
        print("glare seed", seed, "pose diff", dp, dr)
        assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (seed, dp, dr)
        assert np.allclose(res["cov"][i].reshape(6, 6), cov, rtol=1e-6, atol=1e-12), seed


def test_slots_of_256_and_257_spots(hip, orc):
    """A slot with 256 passing spots and one with 257: n == 256 both times, status 0 and -10, the first 256 of the
    oracle's order."""
    K, D = synth.camera_for(GRID_ROWS, GRID_COLS)
    rng = np.random.default_rng(256)
    frames = [grid_frame(rng, 256), grid_frame(rng, 257)]
    roi = (0, 0, GRID_COLS, GRID_ROWS)
    dets, corr, res = hip.track_step_batch_wide(frames, [roi, roi], [None, None], [(M4, K, D, mpe.demo_params())], None)
    for i, (count, status) in enumerate(((256, 0), (257, -10))):
        und, dist = orc.find_leds(frames[i], orc.make_params(), K, D)
        assert len(und) == count
        assert dets["n"][i] == 256 and dets["status"][i] == status and res["status"][i] == (status or 1), (i, dets["n"][i], dets["status"][i])
        assert np.array_equal(dets["undist_xy"][i].reshape(-1, 2), und[:256]) and np.array_equal(dets["dist_xy"][i].reshape(-1, 2), dist[:256])
        assert res["n_corr"][i] == 0 and not corr[i].any()


# ---- 3. the tracker against the oracle's ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["a3", "a4", "b", "c", "d"])
def test_tracker_matches_oracle_through_glare(hip, scenes, name):
    """mpe_tracker_estimate with the switch on, frame by frame against oracle.Tracker: (a) the glare frame is tracked
    over its 107 / 130 ROI detections and the stream tracks on; (b) 68 ROI detections, rows rejected, the wide brute
    force finds nothing, the next frame recovers; (c) start-up over 70 detections finds nothing, frame 1 initialises;
    (d) start-up over 70 detections FINDS the pose, and the stream tracks on from it."""
    s = scenes["seq"][name]
    d = s["d"]
    th = mpe.Tracker(hip, d["markers"], d["K"], d["D"], _params(s["kw"]))
    th.set_wide_frames(True)
    try:
        for k in range(len(s["frames"])):
            ro = s["ref"][k]
            rh = th.estimate(s["frames"][k], s["times"][k])
            for key in KEYS:
                assert rh[key] == ro[key], (name, k, key, rh[key], ro[key])
            if ro["updated"]:
                dp, dr = pose_diff(rh["T"], ro["T"])
                print(name, "frame", k, "pose diff", dp, dr)
                assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (name, k, dp, dr)
                assert np.allclose(rh["cov"], ro["cov"], rtol=1e-6, atol=1e-12), (name, k)
    finally:
        th.close()


def test_switch_is_off_by_default(hip, scenes):
    """The glare frame of (a) ends with MPE_FRAME_TOO_MANY_DETECTIONS for a tracker nobody switched."""
    s = scenes["seq"]["a3"]
    d = s["d"]
    th = mpe.Tracker(hip, d["markers"], d["K"], d["D"], _params(s["kw"]))
    try:
        for k in range(3):
            assert th.estimate(s["frames"][k], s["times"][k])["updated"]
        with pytest.raises(mpe.MpeError, match=r"\(-10\)"):
            th.estimate(s["frames"][3], s["times"][3])
    finally:
        th.close()


# ---- 4. lock step -----------------------------------------------------------------------------------------------------

GROUP = ("a3", "a4", "b", "c")


def _group(scenes):
    """Six streams of two set-ups: the four C1 glare sequences and two clean C2 sequences."""
    streams = [dict(scenes["seq"][n]) for n in GROUP]
    for seed in (31, 32):
        d = synth.make_sequence("C2", N_SEQ, seed)
        streams.append(dict(d=d, frames=d["frames"], times=d["times"], kw=dict(roi_border_thickness=BORDER), glare=None))
    return streams


def _trackers(h, streams, wide):
    ts = [mpe.Tracker(h, s["d"]["markers"], s["d"]["K"], s["d"]["D"], _params(s["kw"])) for s in streams]
    for t in ts:
        t.set_wide_frames(wide)
    return ts


def _per_stream(h, s):
    """mpe_tracker_estimate frame by frame with the switch on, as the records and info the batch entries write."""
    t = _trackers(h, [s], True)[0]
    n = len(s["frames"])
    rec, info = np.zeros(n, mpe.RESULT_DTYPE), np.zeros((n, 8), np.int32)
    for k in range(n):
        f = np.ascontiguousarray(s["frames"][k])
        res, inf = mpe.binding.MpeResult(), (C.c_int * 8)()
        rc = h._lib.mpe_tracker_estimate(t._t, f.ctypes.data, f.shape[0], f.shape[1], f.strides[0], float(s["times"][k]),
                                         C.byref(res), inf)
        assert rc >= 0, (k, rc)
        rec[k] = np.frombuffer(bytes(res), mpe.RESULT_DTYPE)[0]
        info[k] = list(inf)
    t.close()
    return rec, info


def _run_group(h, streams, wide, source):
    ts = _trackers(h, streams, wide)
    times = streams[0]["times"]
    try:
        if source == "host":
            return mpe.tracker_run_sequences_batch_mixed(ts, [s["frames"] for s in streams], times)
        import torch
        enc = "mono8" if source == "device" else "bgr8"
        dev = [torch.from_numpy(np.ascontiguousarray(s["frames"]) if enc == "mono8" else _bgr(s["frames"])).cuda() for s in streams]
        return mpe.tracker_run_sequences_batch_device(ts, dev, times, encoding=enc)
    finally:
        for t in ts:
            t.close()


@pytest.fixture(scope="module")
def group_ref(scenes):
    streams = _group(scenes)
    h = mpe.Handle(0)
    ref = [_per_stream(h, s) for s in streams]
    h.close()
    return streams, np.stack([r for r, _ in ref]), np.stack([i for _, i in ref])


@pytest.mark.parametrize("source", ["host", "device", "bgr8"])
def test_lock_step_group_equals_the_streams_alone(scenes, group_ref, source):
    """Six streams in one group through mpe_tracker_run_sequences_batch_mixed_threads / _device_threads /
    _device_encoded_threads: records and info byte-identical to mpe_tracker_estimate per stream; one wide submission per
    time step that had a glare lane (frame 0: (c); frame 3: both (a) and (b)), "wide_frames" up by the two wide brute
    forces.  With the switch off the same call returns the zeroed -10 records for exactly the glare frames, and
    identical records for every stream up to its glare frame and for the clean streams throughout (a stream that lost
    a frame goes on from another state)."""
    streams, rec_ref, info_ref = group_ref
    h = mpe.Handle(0)
    try:
        c0 = {k: h.get_option(k) for k in ("wide_track_submits", "wide_frames")}
        rec, info = _run_group(h, streams, True, source)
        c1 = {k: h.get_option(k) - c0[k] for k in c0}
        assert rec.tobytes() == rec_ref.tobytes(), np.argwhere(rec["status"] != rec_ref["status"])
        assert np.array_equal(info, info_ref)
        assert c1 == dict(wide_track_submits=2, wide_frames=2), c1
        assert (info[0, 3, 5], info[1, 3, 5], info[2, 3, 5], info[3, 0, 5]) == (107, 130, 68, 70)
        off_rec, off_info = _run_group(h, streams, False, source)
        assert {k: h.get_option(k) - c0[k] for k in c0} == c1            # (nothing wide ran)
        for j, s in enumerate(streams):
            g = s["glare"]
            upto = N_SEQ if g is None else g
            assert off_rec[j, :upto].tobytes() == rec[j, :upto].tobytes() and np.array_equal(off_info[j, :upto], info[j, :upto]), j
            assert [k for k in range(N_SEQ) if off_rec["status"][j, k] == -10] == ([] if g is None else [g]), (j, off_rec["status"][j])
            if g is not None:
                zero = np.zeros(1, mpe.RESULT_DTYPE)
                zero["status"] = -10
                assert off_rec[j, g].tobytes() == zero[0].tobytes() and not off_info[j, g].any(), j
    finally:
        h.close()


# ---- 5. edges ---------------------------------------------------------------------------------------------------------

def test_roi_of_257_rectangles_keeps_its_code(orc, scenes):
    """A tracked stream whose (wide-bordered) ROI holds more than 256 passing rectangles: -10 with the switch on as with
    it off, and the stream is left as the failed call leaves it today — same state, same records afterwards."""
    d = scenes["base"][3]["d"]
    kw = dict(roi_border_thickness=150)
    roi = _oracle_run(orc, d, d["frames"][:4], d["times"][:4], **kw)[3]["roi"]
    f = d["frames"].copy()
    assert paint(f[3], roi, _leds(d, d["T_true"][3]), 14.0, limit=300) == 300
    h = mpe.Handle(0)
    outs = []
    try:
        for wide in (False, True):
            t = mpe.Tracker(h, d["markers"], d["K"], d["D"], _params(kw))
            t.set_wide_frames(wide)
            got = []
            for k in range(N_SEQ):
                if k == 3:
                    with pytest.raises(mpe.MpeError, match=r"\(-10\)"):
                        t.estimate(f[k], d["times"][k])
                    st = C.create_string_buffer(1024)
                    assert h._lib.mpe_tracker_get_state(t._t, st) == 0
                    got.append(st.raw)
                else:
                    r = t.estimate(f[k], d["times"][k])
                    got.append((r["updated"], r["roi"], r["n_det"], r["n_corr"], r["used_bruteforce"], r["T"].tobytes(),
                                r["cov"].tobytes()))
            outs.append(got)
            t.close()
        assert outs[0] == outs[1]
        assert outs[1][2][0] and outs[1][4][0]   # (tracked before, and goes on afterwards)
    finally:
        h.close()


def test_vote_arith_2_keeps_the_code_for_the_wide_brute_lane_only(scenes):
    """Under vote_arith 2 (no strict form) the lane that needs the wide brute force — (b) on frame 3 — keeps -10; the
    other streams of the group, the glare-tracked (a) among them, get their records, and the call does not fail."""
    streams = [dict(scenes["seq"][n]) for n in ("b", "a3")] + [_group(scenes)[4]]
    h = mpe.Handle(0)
    ts = _trackers(h, streams, True)
    try:
        for k in range(4):
            if k == 3:
                h.set_option("vote_arith", 2)
            rec, info, upd = mpe.tracker_estimate_batch_mixed(ts, [s["frames"][k] for s in streams], [streams[0]["times"][k]] * 3)
            if k < 3:
                assert (rec["status"] == 0).all(), (k, rec["status"])
        assert rec["status"].tolist() == [-10, 0, 0] and upd.tolist() == [False, True, True], (rec["status"], upd)
        assert info[1, 5] == 107 and not info[0].any()
    finally:
        h.set_option("vote_arith", 3)
        for t in ts:
            t.close()
        h.close()


def test_usage_errors_leave_the_handle_usable(hip, scenes):
    lib = hip._lib
    d = scenes["base"][3]["d"]
    img = np.ascontiguousarray(d["frames"][1])
    rows, cols = img.shape
    roi = scenes["base"][3]["rec"][1]["roi"]
    pred = np.ascontiguousarray(synth.project(d["T_true"][1], M4, d["K"]))
    K, D, M, P = (np.ascontiguousarray(d["K"], float).reshape(9), np.ascontiguousarray(d["D"], float),
                  np.ascontiguousarray(M4, float), _params(dict(roi_border_thickness=BORDER)))
    su = mpe.binding.TrackSetup(C.addressof(P), K.ctypes.data, D.ctypes.data, len(D), M.ctypes.data, 4)
    item = mpe.binding.TrackItem(img.ctypes.data, *[int(v) for v in roi], pred.ctypes.data)
    dets, corr, res = np.zeros(1, mpe.DETECTIONS_WIDE_DTYPE), np.zeros((1, mpe.MAX_MARKERS, 2), np.uint32), np.zeros(1, mpe.RESULT_DTYPE)
    idx = (C.c_int * 1)(0)
    good = dict(h=hip._h, items=C.byref(item), idx=idx, n=1, rows=rows, cols=cols, stride=cols, dev=0, enc=0, su=C.byref(su), ns=1,
                dets=dets.ctypes.data, corr=corr.ctypes.data, res=res.ctypes.data)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mpe_track_step_batch_wide(a["h"], a["items"], a["idx"], a["n"], a["rows"], a["cols"], C.c_size_t(a["stride"]),
                                             a["dev"], a["enc"], 0, a["su"], a["ns"], C.c_void_p(a["dets"]), C.c_void_p(a["corr"]),
                                             C.c_void_p(a["res"]))

    before = hip.get_option("wide_track_submits")
    for null in ("h", "items", "su", "dets", "corr", "res"):
        assert call(**{null: None}) == -1, null
    assert call(n=-1) == -1 and call(ns=0) == -1 and call(rows=0) == -1 and call(cols=0) == -1
    assert call(idx=None, ns=2) == -1                       # item_setup NULL only with one set-up
    assert call(idx=(C.c_int * 1)(1)) == -1                 # set-up index out of range
    assert call(rows=roi[1] + roi[3] - 1) == -1             # ROI outside the image
    assert call(enc=17) == -3                               # no such encoding
    assert call(enc=1) == -1                                # host frames are mono8
    assert "host frames are mono8" in lib.mpe_last_error(hip._h).decode()   # (named before the stride, short for bgr8)
    assert call(dev=1) == -1                                # a host pointer is no device frame
    assert call(dev=1, enc=1, stride=cols) == -1            # stride below cols * bytes per pixel
    assert call(n=0) == 0
    # an un-collected lock-step submission, an un-collected streaming submission
    dp = C.POINTER(C.c_double)
    rc = lib.mpe_track_step_batch_submit(hip._h, C.byref(item), 1, rows, cols, C.c_size_t(cols), C.byref(P), K.ctypes.data_as(dp),
                                         D.ctypes.data_as(dp), len(D), M.ctypes.data_as(dp), 4)
    assert rc == 0
    try:
        assert call() == -1
    finally:
        assert lib.mpe_track_step_batch_cancel(hip._h) == 0
    import torch
    d_frames = torch.zeros((1, 64, 64), dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(mpe.RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    hip.estimate_batch_device_submit(d_frames.data_ptr(), 1, 64, 64, M4, d["K"], D, P, d_res.data_ptr())
    try:
        assert call() == -1
    finally:
        hip.estimate_batch_device_collect()
        hip.synchronize()
    assert hip.get_option("wide_track_submits") == before     # (nothing reached the device)
    # ... and the handle works
    assert call() == 0 and res["status"][0] == 0 and dets["n"][0] == 4 and res["n_corr"][0] == 4
    assert call(idx=None) == 0 and res["status"][0] == 0
    assert hip.get_option("wide_track_submits") == before + 2


# ---- 6. the facade ----------------------------------------------------------------------------------------------------

def test_facade_tracks_through_glare(scenes, tmp_path):
    """Sequence (a) of seed 3 through compat PoseEstimator::estimateBodyPose with setWideFrames(true)
    (compat/facade_wide_tracking): no exception, and on every frame the oracle's update flag, ROI, detection and row
    counts, pose and covariance.  With the switch off the glare frame raises the capacity exception, as today."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "compat")])
    s = scenes["seq"]["a3"]
    d = s["d"]
    yaml, raw = str(tmp_path / "m4.yaml"), str(tmp_path / "frames.raw")
    with open(yaml, "w") as fh:
        fh.write("marker_positions:\n")
        for m in d["markers"]:
            fh.write("  - x: %.17g\n    y: %.17g\n    z: %.17g\n" % tuple(m))
    np.ascontiguousarray(s["frames"]).tofile(raw)
    K = d["K"]
    args = [os.path.join(root, "compat", "facade_wide_tracking"), "--markers", yaml, "--frames", raw, "--rows", str(d["rows"]),
            "--cols", str(d["cols"]), "--n", str(N_SEQ), "--dt", repr(float(s["times"][1] - s["times"][0])), "--camera",
            "%.17g %.17g %.17g %.17g" % (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), "--dist", " ".join("%.17g" % v for v in d["D"]),
            "--border", str(BORDER)]

    def run(wide):
        out = subprocess.run(args + ["--wide", str(wide)], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stdout[-800:], out.stderr[-800:])
        return out.stdout.splitlines()

    lines = run(1)
    assert not any("exception" in ln for ln in lines), lines
    for k, ro in enumerate(s["ref"]):
        head = "frame %d updated %d roi %d %d %d %d points %d rows %d" % ((k, int(ro["updated"])) + tuple(ro["roi"]) +
                                                                          (ro["n_det"], ro["n_corr"]))
        assert head in lines, (k, head, [ln for ln in lines if ln.startswith("frame %d updated" % k)])
        vals = {ln.split()[2]: np.array(ln.split()[3:], float) for ln in lines if ln.startswith("frame %d " % k) and
                ln.split()[2] in ("pose", "cov")}
        dp, dr = pose_diff(vals["pose"].reshape(4, 4), ro["T"])
        assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (k, dp, dr)
        assert np.allclose(vals["cov"].reshape(6, 6), ro["cov"], rtol=1e-6, atol=1e-12), k
    off = run(0)
    assert any(ln.startswith("frame 3 exception") for ln in off), off
    assert "frame 2 updated 1 roi %d %d %d %d points 4 rows 4" % tuple(s["ref"][2]["roi"]) in off, off
