"""Lock-step tracking of streams whose camera, marker set and parameters differ (mpe_track_step_batch_setups,
mpe_tracker_estimate_batch_mixed, mpe_tracker_run_sequences_batch_mixed_threads): the cameras of a multi-camera rig
in ONE device submission per time step.  Every stream must give the records of its set-up run as a uniform group."""
import ctypes
import hashlib

import numpy as np
import pytest

from rpg_monocular_pose_estimator_amd import synth
import rpg_monocular_pose_estimator_amd as mpe
from util import pose_diff, POS_TOL_M, ROT_TOL_RAD

NEW_SYMBOLS = ("mpe_track_step_batch_setups", "mpe_track_step_batch_setups_submit", "mpe_tracker_estimate_batch_mixed",
               "mpe_tracker_run_sequences_batch_mixed_threads")


@pytest.fixture(scope="module")
def lib():
    mpe.build_library()
    return mpe.load_library()


# ---- CPU tier -----------------------------------------------------------------------------------------------------

def test_mixed_entries_are_exported(lib):
    names = mpe.exported_symbols()
    for s in NEW_SYMBOLS:
        assert s in names, s
        assert hasattr(lib, s), s


def test_mixed_entries_reject_bad_usage_without_a_device(lib):
    """Null pointers, duplicated trackers and trackers of different handles: MPE_ERR_ARG before any device work."""
    fr = np.zeros((2, 16, 16), np.uint8)
    ptrs = (ctypes.c_void_p * 2)(fr.ctypes.data, fr.ctypes.data)
    times = np.zeros(2)
    dp = times.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    null_ts = (ctypes.c_void_p * 1)(None)
    # mpe_track_step_batch_setups[_submit]: no handle
    setup_idx = (ctypes.c_int * 1)(0)
    assert lib.mpe_track_step_batch_setups_submit(None, None, setup_idx, 1, 16, 16, ctypes.c_size_t(16), None, 1) == -1
    assert lib.mpe_track_step_batch_setups(None, None, setup_idx, 1, 16, 16, ctypes.c_size_t(16), None, 1,
                                           None, None, None) == -1
    # mpe_tracker_estimate_batch_mixed
    call = lib.mpe_tracker_estimate_batch_mixed
    assert call(None, 1, ptrs, 16, 16, 16, dp, None, None, None) == -1           # no trackers
    assert call(null_ts, 1, ptrs, 16, 16, 16, dp, None, None, None) == -1        # null tracker
    assert call(null_ts, 0, ptrs, 16, 16, 16, dp, None, None, None) == 0         # nothing to do
    # mpe_tracker_run_sequences_batch_mixed_threads
    run = lib.mpe_tracker_run_sequences_batch_mixed_threads
    assert run(None, 1, ptrs, 2, 16, 16, 16, 256, dp, None, None, 2) == -1       # no trackers
    assert run(null_ts, 1, ptrs, 2, 16, 16, 16, 256, dp, None, None, 2) == -1    # null tracker
    assert run(null_ts, 1, ptrs, 2, 16, 16, 16, 256, dp, None, None, 0) == -1    # n_threads < 1
    assert run(null_ts, 0, ptrs, 2, 16, 16, 16, 256, dp, None, None, 1) == 0     # nothing to do
    # trackers only remember their handle until a frame is processed: two stand-in handles that are never touched
    fake = [ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)]
    ts = []
    for f in fake:
        t = ctypes.c_void_p()
        assert lib.mpe_tracker_create(ctypes.addressof(f), ctypes.byref(t)) == 0
        ts.append(t)
    try:
        other = (ctypes.c_void_p * 2)(ts[0].value, ts[1].value)
        dup = (ctypes.c_void_p * 2)(ts[0].value, ts[0].value)
        assert call(other, 2, ptrs, 16, 16, 16, dp, None, None, None) == -1      # different handles
        assert call(dup, 2, ptrs, 16, 16, 16, dp, None, None, None) == -1        # the same tracker twice
        assert run(dup, 2, ptrs, 2, 16, 16, 16, 256, dp, None, None, 1) == -1    # the same tracker twice in a group
    finally:
        for t in ts:
            lib.mpe_tracker_destroy(t)


def _sequence_digest(d):
    h = hashlib.sha256()
    for k in ("frames", "T_true", "times", "K", "D", "markers"):
        h.update(np.ascontiguousarray(d[k]).tobytes())
    return h.hexdigest()


def test_make_sequence_default_camera_unchanged():
    """camera=None renders exactly what make_sequence rendered before it took a camera (digest of that output)."""
    d = synth.make_sequence("C2", 4, seed=21, dropout=(2,), salt=0.001)
    assert _sequence_digest(d) == "091dff270edcd91c580ed92cf845291a22942f899da032bc729de4c558540386"
    assert _sequence_digest(synth.make_sequence("C2", 4, seed=21, dropout=(2,), salt=0.001, camera=None)) == \
        _sequence_digest(d)


def _camera_b():
    K = synth.README_K.copy()
    K[0, 0] *= 1.1
    K[1, 1] *= 1.1
    K[0, 2] += 14.0
    K[1, 2] -= 9.0
    return K, np.array([-0.30, 0.12, 0.0003, -0.0001, 0.0])


def _camera_c():
    K = synth.README_K.copy()
    K[0, 0] *= 0.95
    K[1, 1] *= 0.95
    K[0, 2] -= 11.0
    K[1, 2] += 7.0
    return K, np.array([-0.40, 0.18, -0.0004, 0.0002, -0.01])


def test_make_sequence_camera_override_renders_another_image():
    a = synth.make_sequence("C2", 3, seed=33)
    K, D = _camera_b()
    b = synth.make_sequence("C2", 3, seed=33, camera=(K, D))
    assert np.array_equal(b["K"], K) and np.array_equal(b["D"], D)
    assert not np.array_equal(a["frames"], b["frames"])


# ---- GPU tier -----------------------------------------------------------------------------------------------------

M10 = np.vstack([synth.M8, [[0.0600, 0.0500, 0.0300], [-0.0800, 0.0100, 0.0700]]])
N_FRAMES = 24


def _setups():
    """(name, config, camera or None, parameter overrides): six set-ups, one of them with more than 8 markers."""
    kw4 = dict(threshold_value=120, gaussian_sigma=0.8, nearest_neighbour_pixel_tolerance=6.0,
               back_projection_pixel_tolerance=4.0)
    c10 = dict(synth.CONFIGS["C2"], markers=M10)
    return [("C2 README camera", "C2", None, {}),
            ("C2 camera B", "C2", _camera_b(), {}),
            ("M4 camera C", "C1", _camera_c(), {}),
            ("M8 README camera", "C3", None, {}),
            ("C2 other parameters", "C2", None, kw4),
            ("10 markers", c10, None, {})]


def _data_set():
    """Two streams per set-up, listed interleaved (stream j has set-up j % 6).  Drop-outs at the same frames in two
    set-ups (whole-image retries, then re-initialisations at the same time step); one salt stream overflows the small
    blob tier inside the mixed submission."""
    S = _setups()
    n_s = 2 * len(S)
    drop = {1: (9,), 2: (9,), 3: (15,), 4: (15,), 11: (18,)}
    seqs = []
    for j in range(n_s):
        name, cfg, cam, kw = S[j % len(S)]
        seqs.append(synth.make_sequence(cfg, N_FRAMES, seed=900 + j, dropout=drop.get(j, ()), camera=cam,
                                        salt=0.002 if j == 6 else 0.0))
    return S, seqs


def _trackers(handles, S, seqs, which=None):
    out = []
    for j, q in enumerate(seqs):
        kw = S[j % len(S)][3]
        h = handles[j % len(handles)] if which is None else handles[which(j)]
        out.append(mpe.Tracker(h, q["markers"], q["K"], q["D"], mpe.demo_params(**kw)))
    return out


def _close(ts, hs):
    for t in ts:
        t.close()
    for h in hs:
        h.close()


@pytest.fixture(scope="module")
def mixed_run():
    S, seqs = _data_set()
    h = mpe.Handle(0)
    ts = _trackers([h], S, seqs)
    c0 = {k: h.get_option(k) for k in ("track_batch_submits", "track_batch_chains", "track_batch_reruns")}
    rec, info = mpe.tracker_run_sequences_batch_mixed(ts, [q["frames"] for q in seqs], seqs[0]["times"])
    c1 = {k: h.get_option(k) - c0[k] for k in c0}
    _close(ts, [h])
    return dict(S=S, seqs=seqs, rec=rec, info=info, counters=c1)


@pytest.mark.gpu
def test_mixed_group_equals_uniform_groups(mixed_run):
    """Byte-identical records and info to each set-up's streams as a uniform group on a handle of its own."""
    S, seqs = mixed_run["S"], mixed_run["seqs"]
    hs = [mpe.Handle(0) for _ in S]
    ts = _trackers(hs, S, seqs)
    rec, info = mpe.tracker_run_sequences_batch(ts, [q["frames"] for q in seqs], seqs[0]["times"])
    c = {k: sum(h.get_option(k) for h in hs) for k in ("track_batch_chains", "track_batch_reruns")}
    _close(ts, hs)
    assert rec.tobytes() == mixed_run["rec"].tobytes()
    assert np.array_equal(info, mixed_run["info"])
    # the uniform groups take the same rare paths as the mixed one, and count them alike
    assert c["track_batch_reruns"] >= 1, c                    # the salt stream overflowed the small tier
    assert c["track_batch_chains"] >= N_FRAMES, c             # the 10-marker set-up: the chain of kernels every step


@pytest.mark.gpu
def test_mixed_group_matches_oracle(mixed_run, orc):
    """Every stream against orc.Tracker with its own camera, markers and parameters; the drop-outs produce whole-image
    retries and re-initialisations in two set-ups at the same time step, and the salt stream a re-run."""
    S, seqs, rec, info = mixed_run["S"], mixed_run["seqs"], mixed_run["rec"], mixed_run["info"]
    cols = seqs[0]["cols"]
    for j, q in enumerate(seqs):
        to = orc.Tracker(q["markers"], q["K"], q["D"], orc.make_params(**S[j % len(S)][3]))
        for k in range(N_FRAMES):
            ro = to.estimate(q["frames"][k], q["times"][k])
            assert rec["status"][j, k] >= 0, (j, k, rec["status"][j, k])
            assert (rec["status"][j, k] == 0) == ro["updated"], (j, k)
            assert tuple(info[j, k, 0:4]) == ro["roi"] and info[j, k, 4] == ro["it_since_initialized"], (j, k)
            assert info[j, k, 5] == ro["n_det"] and info[j, k, 6] == ro["n_corr"], (j, k)
            assert bool(info[j, k, 7]) == ro["used_bruteforce"], (j, k)
            if ro["updated"]:
                dp, dr = pose_diff(rec["T"][j, k].reshape(4, 4), ro["T"])
                assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (j, k, dp, dr)
    setup_of = np.arange(len(seqs)) % len(S)
    retry = (info[:, 1:, 2] == cols) & (info[:, 1:, 4] >= 1)   # whole-image ROI while tracking
    brute = info[:, 1:, 7] == 1
    assert max(len(set(setup_of[retry[:, k]])) for k in range(N_FRAMES - 1)) >= 2
    assert max(len(set(setup_of[brute[:, k]])) for k in range(N_FRAMES - 1)) >= 2
    c = mixed_run["counters"]
    assert c["track_batch_reruns"] >= 1, c                    # the salt stream overflowed the small tier
    assert c["track_batch_chains"] >= N_FRAMES, c             # the 10-marker set-up: the chain of kernels every step
    # the streams of the set-ups of 4 .. 8 markers pose most of their frames (the 10-marker object of this data set is
    # never initialised — by the oracle neither: its steps exercise the chain of kernels on detection-only slots)
    tracked = setup_of < 5
    assert int((rec["status"][tracked] == 0).sum()) >= int(tracked.sum()) * (N_FRAMES - 6)


@pytest.mark.gpu
def test_mixed_per_step_entry_equals_loop(mixed_run):
    S, seqs = mixed_run["S"], mixed_run["seqs"]
    h = mpe.Handle(0)
    ts = _trackers([h], S, seqs)
    for k in range(N_FRAMES):
        r, i, upd = mpe.tracker_estimate_batch_mixed(ts, [q["frames"][k] for q in seqs], [seqs[0]["times"][k]] * len(seqs))
        assert r.tobytes() == mixed_run["rec"][:, k].tobytes() and np.array_equal(i, mixed_run["info"][:, k]), k
        assert np.array_equal(upd, r["status"] == 0), k
    _close(ts, [h])


@pytest.mark.gpu
def test_mixed_group_unfused_equals_fused(mixed_run):
    S, seqs = mixed_run["S"], mixed_run["seqs"]
    h = mpe.Handle(0)
    h.set_option("track_fused", 0)
    ts = _trackers([h], S, seqs)
    rec, info = mpe.tracker_run_sequences_batch_mixed(ts, [q["frames"] for q in seqs], seqs[0]["times"])
    _close(ts, [h])
    assert rec.tobytes() == mixed_run["rec"].tobytes() and np.array_equal(info, mixed_run["info"])


@pytest.mark.gpu
def test_mixed_groups_on_two_threads(mixed_run):
    S, seqs = mixed_run["S"], mixed_run["seqs"]
    hs = [mpe.Handle(0), mpe.Handle(0)]
    ts = _trackers(hs, S, seqs, which=lambda j: (j // 3) % 2)   # both handles carry several set-ups
    rec, info = mpe.tracker_run_sequences_batch_mixed(ts, [q["frames"] for q in seqs], seqs[0]["times"], threads=2)
    _close(ts, hs)
    assert rec.tobytes() == mixed_run["rec"].tobytes() and np.array_equal(info, mixed_run["info"])


@pytest.mark.gpu
def test_mixed_entry_with_one_setup_equals_uniform_entry():
    n_s, n = 6, 20
    drop = {2: (8,), 4: (12,)}
    seqs = [synth.make_sequence("C2", n, seed=950 + s, dropout=drop.get(s, ())) for s in range(n_s)]
    frames, times = [q["frames"] for q in seqs], seqs[0]["times"]
    out = []
    for mixed in (False, True):
        h = mpe.Handle(0)
        ts = [mpe.Tracker(h, q["markers"], q["K"], q["D"], mpe.demo_params()) for q in seqs]
        out.append(mpe.tracker_run_sequences_batch(ts, frames, times, mixed=mixed))
        _close(ts, [h])
    assert out[0][0].tobytes() == out[1][0].tobytes() and np.array_equal(out[0][1], out[1][1])


class _TrackItem(ctypes.Structure):  # mpe_track_item
    _fields_ = [("img", ctypes.c_void_p), ("roi_x", ctypes.c_int), ("roi_y", ctypes.c_int), ("roi_w", ctypes.c_int),
                ("roi_h", ctypes.c_int), ("predicted_px", ctypes.c_void_p)]


class _TrackSetup(ctypes.Structure):  # mpe_track_setup
    _fields_ = [("p", ctypes.c_void_p), ("K", ctypes.c_void_p), ("D", ctypes.c_void_p), ("nD", ctypes.c_int),
                ("markers_xyz", ctypes.c_void_p), ("n_markers", ctypes.c_int)]


@pytest.mark.gpu
def test_submit_entries_refuse_bad_usage_and_stay_usable():
    """Usage errors of both submit entries on a real handle: their codes and messages, no submission counted, and the
    handle still takes a valid submit + collect afterwards, whose records are those of the first valid one."""
    lib = mpe.load_library()
    q = synth.make_sequence("C2", 1, seed=990)
    rows, cols = int(q["rows"]), int(q["cols"])
    img = np.ascontiguousarray(q["frames"][0])
    K, D = np.ascontiguousarray(q["K"], np.float64), np.ascontiguousarray(q["D"], np.float64)
    markers = np.ascontiguousarray(q["markers"], np.float64)
    m17 = np.zeros((17, 3))
    P, P_sigma0 = mpe.demo_params(), mpe.demo_params(gaussian_sigma=0.0)
    pred = np.ascontiguousarray(synth.project(q["T_true"][0], q["markers"], q["K"]), np.float64)
    px = synth.distort_px(pred, q["K"], q["D"])
    x0, y0 = [max(0, int(v) - 40) for v in px.min(0)]
    x1, y1 = min(cols, int(px[:, 0].max()) + 40), min(rows, int(px[:, 1].max()) + 40)
    h = mpe.Handle(0)
    hp = h._h
    trackers = []

    def items(roi_x=0):
        it = (_TrackItem * 2)()
        it[0] = _TrackItem(img.ctypes.data, roi_x, 0, cols, rows, None)                     # whole image, detection only
        it[1] = _TrackItem(img.ctypes.data, x0, y0, x1 - x0, y1 - y0, pred.ctypes.data)      # tracked around the LEDs
        return it

    def ptr(a):
        return ctypes.c_void_p(a.ctypes.data)

    def submit(it, p=P, mk=markers, n_markers=len(markers)):
        return lib.mpe_track_step_batch_submit(hp, it, 2, rows, cols, ctypes.c_size_t(img.strides[0]), ctypes.byref(p),
                                               ptr(K), ptr(D), len(D), ptr(mk), n_markers)

    def submit_setups(it, idx=(0, 0), mk=markers, n_markers=len(markers)):
        su = (_TrackSetup * 1)(_TrackSetup(ctypes.addressof(P), K.ctypes.data, D.ctypes.data, len(D), mk.ctypes.data,
                                           n_markers))
        return lib.mpe_track_step_batch_setups_submit(hp, it, (ctypes.c_int * 2)(*idx), 2, rows, cols,
                                                      ctypes.c_size_t(img.strides[0]), su, 1)

    def collect():
        dets, corr, res = np.zeros(2, mpe.DETECTIONS_DTYPE), np.zeros(2 * 32, np.uint32), np.zeros(2, mpe.RESULT_DTYPE)
        assert lib.mpe_track_step_batch_collect(hp, ptr(dets), ptr(corr), ptr(res)) == 0
        return dets.tobytes() + corr.tobytes() + res.tobytes()

    def refused(rc, code, text):
        assert rc == code, (rc, code, text)
        assert text in lib.mpe_last_error(hp).decode(), lib.mpe_last_error(hp).decode()

    try:
        assert submit(items()) == 0
        ref = collect()
        n0 = h.get_option("track_batch_submits")
        cases = [(submit, dict(it=items(roi_x=1)), -1, "ROI outside the image"),
                 (submit, dict(it=items(), mk=m17, n_markers=17), -3, "n_markers > MPE_MAX_MARKERS"),
                 (submit, dict(it=items(), p=P_sigma0), -1, "gaussian_sigma must be in (0, 6]"),
                 (submit_setups, dict(it=items(), idx=(0, 1)), -1, "set-up index out of range"),
                 (submit_setups, dict(it=items(), idx=(-1, 0)), -1, "set-up index out of range"),
                 (submit_setups, dict(it=items(), mk=m17, n_markers=17), -1, "set-up with n_markers > MPE_MAX_MARKERS")]
        for entry, kw, code, text in cases:
            refused(entry(**kw), code, text)
            assert h.get_option("track_batch_submits") == n0, text
            assert entry(items()) == 0, text
            assert collect() == ref, text
            n0 += 1
        for entry in (submit, submit_setups):   # a second submit while one is pending
            assert entry(items()) == 0
            refused(submit(items()), -1, "a submitted batch has not been collected yet")
            refused(submit_setups(items()), -1, "a submitted batch has not been collected yet")
            assert collect() == ref
            assert entry(items()) == 0 and collect() == ref
        assert h.get_option("track_batch_submits") == n0 + 4
        # while a submission is pending, a tracked frame, a lone tracker on either branch and a lock-step call are
        # refused, and none of them touches that submission
        trackers += [mpe.Tracker(h, markers, K, D, P), mpe.Tracker(h, markers, K, D, P)]
        fresh, tracking = trackers
        assert tracking.estimate(img, 0.0)["it_since_initialized"] >= 1
        # (that frame was a submission of one slot: the bytes of a record beyond its valid entries are what the device
        #  buffer last held there, so the reference records are taken again)
        assert submit(items()) == 0
        ref = collect()
        calls = [("mpe_track_step", lambda: h.track_step(img, (x0, y0, x1 - x0, y1 - y0), P, K, D, markers, pred)),
                 ("uninitialised tracker", lambda: fresh.estimate(img, 0.1)),
                 ("tracking tracker", lambda: tracking.estimate(img, 0.1)),
                 ("mpe_tracker_estimate_batch", lambda: mpe.tracker_estimate_batch(trackers, [img, img], [0.1, 0.1]))]
        for what, call in calls:
            assert submit(items()) == 0
            with pytest.raises(mpe.MpeError, match=r"\(-1\): a submitted batch has not been collected yet"):
                call()
            assert collect() == ref, what
    finally:
        lib.mpe_track_step_batch_cancel(hp)
        for t in trackers:
            t.close()
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [True, False], ids=["mixed", "uniform"])
def test_mixed_steady_state_step_is_one_submission(mixed):
    """A time step on which every stream is tracking and none retries, re-initialises or needs the large size class
    costs the whole mixed group (three set-ups: two cameras, two parameter sets) exactly one device submission — one
    launch of k_track_frame — and no chain of kernels.  So does a uniform group of as many streams (one set-up)."""
    S = [_setups()[i] for i in ((0, 1, 4) if mixed else (0,))]
    seqs = []
    for j in range(9):
        name, cfg, cam, kw = S[j % len(S)]
        seqs.append(synth.make_sequence(cfg, 16, seed=970 + j, camera=cam))
    h = mpe.Handle(0)
    ts = _trackers([h], S, seqs)
    rows, cols = seqs[0]["rows"], seqs[0]["cols"]
    n_steady = 0
    prev_it = np.zeros(len(seqs), int)
    names = ("track_batch_submits", "track_batch_chains", "track_batch_reruns")
    seen = []
    for k in range(16):
        c0 = [h.get_option(x) for x in names]
        r, info, upd = mpe.tracker_estimate_batch(ts, [q["frames"][k] for q in seqs], [seqs[0]["times"][k]] * len(seqs),
                                                  mixed=mixed)
        d = [h.get_option(x) - c for x, c in zip(names, c0)]
        small = (info[:, 2].astype(np.int64) * info[:, 3] * 4 <= rows * cols).all()
        seen.append((k, d, prev_it.tolist(), bool(small), int(info[:, 7].sum())))
        if (prev_it >= 1).all() and small and not info[:, 7].any():
            assert d == [1, 0, 0], (k, d)
            n_steady += 1
        prev_it = info[:, 4].copy()
    _close(ts, [h])
    assert n_steady >= 8, seen
