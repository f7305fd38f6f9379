"""Lock-step tracking of streams whose frames are in DEVICE memory (mpe_track_step_batch_setups_device[_submit],
mpe_tracker_estimate_batch_device, mpe_tracker_run_sequences_batch_device_threads): a kernel gathers every stream's ROI
from the caller's device image into the slot the host entries pack and copy, so every record must equal the host
entries' byte for byte.  CPU tier: exports, usage errors, and the gather arithmetic compiled for the host and run
under AddressSanitizer; GPU tier: the stage entry, the tracker entries and usage errors on a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from rpg_monocular_pose_estimator_amd import synth
import rpg_monocular_pose_estimator_amd as mpe
from util import pose_diff, POS_TOL_M, ROT_TOL_RAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")
NEW_SYMBOLS = ("mpe_track_step_batch_setups_device", "mpe_track_step_batch_setups_device_submit",
               "mpe_tracker_estimate_batch_device", "mpe_tracker_run_sequences_batch_device_threads")


@pytest.fixture(scope="module")
def lib():
    mpe.build_library()
    return mpe.load_library()


# ---- CPU tier -----------------------------------------------------------------------------------------------------

def test_device_frame_entries_are_exported(lib):
    names = mpe.exported_symbols()
    for s in NEW_SYMBOLS:
        assert s in names, s
        assert hasattr(lib, s), s
    for s in ("tracker_estimate_batch_device", "tracker_run_sequences_batch_device"):
        assert callable(getattr(mpe, s)), s
    assert callable(mpe.Handle.track_step_batch_device)


def test_device_frame_entries_reject_bad_usage_without_a_device(lib):
    """Null handle, null trackers, duplicates, trackers of different handles, n == 0 and n_threads < 1: refused (or
    nothing to do) before any device work, as the host-frame entries refuse them."""
    fr = np.zeros((2, 16, 16), np.uint8)     # (never read: every call is refused before it looks at a frame)
    ptrs = (ctypes.c_void_p * 2)(fr.ctypes.data, fr.ctypes.data)
    times = np.zeros(2)
    dp = times.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    null_ts = (ctypes.c_void_p * 1)(None)
    setup_idx = (ctypes.c_int * 1)(0)
    assert lib.mpe_track_step_batch_setups_device_submit(None, None, setup_idx, 1, 16, 16, 16, None, 1) == -1
    assert lib.mpe_track_step_batch_setups_device_submit(None, None, None, 1, 16, 16, 16, None, 1) == -1
    assert lib.mpe_track_step_batch_setups_device(None, None, setup_idx, 1, 16, 16, 16, None, 1, None, None, None) == -1
    call = lib.mpe_tracker_estimate_batch_device
    assert call(None, 1, ptrs, 16, 16, 16, dp, None, None, None) == -1           # no trackers
    assert call(null_ts, 1, ptrs, 16, 16, 16, dp, None, None, None) == -1        # null tracker
    assert call(null_ts, 1, None, 16, 16, 16, dp, None, None, None) == -1        # no frames
    assert call(null_ts, 0, ptrs, 16, 16, 16, dp, None, None, None) == 0         # nothing to do
    run = lib.mpe_tracker_run_sequences_batch_device_threads
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


def test_gather_arithmetic_on_the_host_under_sanitizers(tmp_path):
    """csrc/mpe_gather.h — what k_gather_rois computes per 16-byte segment — as a stand-alone host program built with
    AddressSanitizer + UBSan: 2 000 seeded cases (images 1 x 1 .. 48 x 64, stride = cols + {0, 1, 3, 16}, base 0 .. 3
    bytes into a heap buffer that ends with the image, ROIs at every corner / whole image / widths 1 .. 17 / widths no
    multiple of 16, slots larger than the ROI), every slot compared byte for byte with a per-byte copy + zero fill.  A
    load outside the image aborts the program (its checked loads, and the sanitizer behind the buffer)."""
    exe = str(tmp_path / "gather_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "tests", "host", "stub"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "gather_host.cpp"), "-o", exe])
    r = subprocess.run([exe, "2000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gather_host ok: 2000 cases" in r.stdout, r.stdout


# ---- GPU tier -----------------------------------------------------------------------------------------------------

N_FRAMES = 24
GUARD = 255


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


def _guarded(img, stride, base):
    """img inside a buffer of GUARD bytes: `base` bytes in front of it, rows `stride` bytes apart, a row of GUARD behind.
    -> (buffer, view of the image in it)"""
    rows, cols = img.shape
    buf = np.full(base + rows * stride + stride, GUARD, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[base:], (rows, cols), (stride, 1))
    view[:] = img
    return buf, view


def _stage_case(salt):
    """5 items of two set-ups over two frames: a ROI at each image corner that reaches over the LEDs (so each is
    tracked to a pose), one of them with odd roi_x and a width that is no multiple of 4, and a whole-image item
    without predicted pixels."""
    qa = synth.make_sequence("C2", 1, seed=1990, salt=salt)
    qb = synth.make_sequence("C2", 1, seed=1991, camera=_camera_b())
    rows, cols = int(qa["rows"]), int(qa["cols"])
    stride, base = cols + 3, 2 * (cols + 3) + 1          # rows no multiple of 4 apart, base pointer odd
    setups = [(q["markers"], q["K"], q["D"], mpe.demo_params()) for q in (qa, qb)]
    rois, preds, which = [], [], []
    for corner in range(4):
        q = (qa, qb)[corner % 2]
        pred = synth.project(q["T_true"][0], q["markers"], q["K"])
        px = synth.distort_px(pred, q["K"], q["D"])
        lo = np.maximum(px.min(0).astype(int) - 40, 0)
        hi = np.minimum(px.max(0).astype(int) + 40, [cols, rows])
        x0, x1 = (0, hi[0]) if corner % 2 == 0 else (lo[0] | 1, cols)
        y0, y1 = (0, hi[1]) if corner < 2 else (lo[1], rows)
        rois.append((int(x0), int(y0), int(x1 - x0), int(y1 - y0)))
        preds.append(pred)
        which.append(corner % 2)
    assert rois[1][0] % 2 == 1 and rois[1][2] % 4 != 0 and rois[3][0] % 2 == 1
    rois.append((0, 0, cols, rows))
    preds.append(None)
    which.append(0)
    return dict(frames=[qa["frames"][0], qb["frames"][0]], rows=rows, cols=cols, stride=stride, base=base, setups=setups,
                rois=rois, preds=preds, which=which)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["fused", "chain", "overflow"])
def test_stage_entry_equals_host_entry(variant):
    """One time step through mpe_track_step_batch_setups (host frames) and mpe_track_step_batch_setups_device (the same
    buffers uploaded): detections, correspondences and records equal as bytes.  The frames sit in buffers of 255-valued
    guard bytes, rows cols + 3 bytes apart, the image an odd number of bytes into its tensor: a window that is off by a
    byte shows as detections.  chain: track_fused 0 (the chain of kernels); overflow: a salt-noise frame, whose slots
    overflow the small blob tier and are re-run in _collect from the gathered slots."""
    import torch
    c = _stage_case(salt=0.002 if variant == "overflow" else 0.0)
    rows, cols, stride, base = c["rows"], c["cols"], c["stride"], c["base"]
    host = [_guarded(f, stride, base) for f in c["frames"]]
    dev_bufs = [torch.from_numpy(buf).cuda() for buf, _ in host]
    dev = [torch.as_strided(t, (rows, cols), (stride, 1), base) for t in dev_bufs]
    assert dev[0].data_ptr() % 2 == 1
    h = mpe.Handle(0)
    try:
        if variant == "chain":
            h.set_option("track_fused", 0)
        names = ("track_batch_submits", "track_batch_chains", "track_batch_reruns")
        out, counts = [], []
        for entry in ("host", "device", "host"):
            c0 = [h.get_option(k) for k in names]
            if entry == "host":
                r = h.track_step_batch([host[w][1] for w in c["which"]], c["rois"], c["preds"], c["setups"], c["which"])
            else:
                r = h.track_step_batch_device([dev[w] for w in c["which"]], c["rois"], c["preds"], c["setups"], c["which"])
            out.append(r)
            counts.append([h.get_option(k) - v for k, v in zip(names, c0)])
        for k, what in enumerate(("detections", "correspondences", "records")):
            assert out[0][k].tobytes() == out[2][k].tobytes(), what    # (the host entry repeats itself)
            assert out[1][k].tobytes() == out[0][k].tobytes(), what
        assert counts[1] == counts[0], counts
        assert counts[1][0] == 1
        dets, corr, res = out[1]
        if variant == "overflow":
            assert counts[1][2] >= 1, counts
        else:
            assert counts[1][1] == (2 if variant == "chain" else 0), counts
            assert (res["status"][:4] == 0).all(), res["status"]            # every corner ROI was tracked to a pose
            assert (dets["n"][:4] == 5).all() and dets["n"][4] == 5, dets["n"]
            assert res["status"][4] == 1                                    # detection only
        # a uniform batch is the submission of one set-up without an index array
        a = [i for i, w in enumerate(c["which"]) if w == 0]
        pick = lambda xs: [xs[i] for i in a]
        u_host = h.track_step_batch([host[0][1]] * len(a), pick(c["rois"]), pick(c["preds"]), c["setups"][:1], [0] * len(a))
        u_dev = h.track_step_batch_device([dev[0]] * len(a), pick(c["rois"]), pick(c["preds"]), c["setups"][:1], None)
        for k in range(3):
            assert u_dev[k].tobytes() == u_host[k].tobytes(), k
        # (compared field by field: what lies beyond a record's valid entries depends on the submission's size)
        assert np.array_equal(u_dev[0]["n"], dets["n"][a]) and np.array_equal(u_dev[2]["status"], res["status"][a])
        assert np.array_equal(u_dev[2]["T"][u_dev[2]["status"] == 0], res["T"][a][res["status"][a] == 0])
    finally:
        h.close()


def _run_both(seqs, params):
    """The sequences through the host-frame entry and through the device-frame entry, fresh trackers on a handle each."""
    import torch
    frames, times = [q["frames"] for q in seqs], seqs[0]["times"]
    out = {}
    for where in ("host", "device"):
        h = mpe.Handle(0)
        ts = [mpe.Tracker(h, q["markers"], q["K"], q["D"], mpe.demo_params(**kw)) for q, kw in zip(seqs, params)]
        if where == "host":
            out[where] = mpe.tracker_run_sequences_batch_mixed(ts, frames, times)
        else:
            d_frames = torch.from_numpy(np.stack(frames)).cuda()
            c0 = h.get_option("track_batch_submits")
            out[where] = mpe.tracker_run_sequences_batch_device(ts, d_frames, times)
            assert h.get_option("track_batch_submits") - c0 >= len(times)
            # the per-step entry gives the records of the loop
            ts2 = [mpe.Tracker(h, q["markers"], q["K"], q["D"], mpe.demo_params(**kw)) for q, kw in zip(seqs, params)]
            ts += ts2
            for k in range(len(times)):
                r, i, upd = mpe.tracker_estimate_batch_device(ts2, [f[k] for f in d_frames], [times[k]] * len(seqs))
                assert r.tobytes() == out[where][0][:, k].tobytes() and np.array_equal(i, out[where][1][:, k]), k
                assert np.array_equal(upd, r["status"] == 0), k
        for t in ts:
            t.close()
        h.close()
    return out


@pytest.mark.gpu
def test_uniform_device_sequences_equal_host_sequences_and_oracle(orc):
    """5 streams of one set-up, 24 frames, LED drop-outs: whole-image retries and brute-force re-initialisations occur
    (4 and 2 with these seeds, by the oracle).  Records and info of the device-frame entries equal those of the
    host-frame entries as bytes, and every frame equals the oracle's state machine."""
    drop = {1: (9,), 3: (14, 15)}
    seqs = [synth.make_sequence("C2", N_FRAMES, seed=950 + s, dropout=drop.get(s, ())) for s in range(5)]
    out = _run_both(seqs, [{}] * 5)
    rec, info = out["device"]
    assert rec.tobytes() == out["host"][0].tobytes()
    assert np.array_equal(info, out["host"][1])
    for s, q in enumerate(seqs):
        to = orc.Tracker(q["markers"], q["K"], q["D"], orc.make_params())
        for k in range(N_FRAMES):
            ro = to.estimate(q["frames"][k], q["times"][k])
            assert (rec["status"][s, k] == 0) == ro["updated"], (s, k)
            assert tuple(info[s, k, 0:4]) == ro["roi"] and info[s, k, 4] == ro["it_since_initialized"], (s, k)
            assert info[s, k, 5] == ro["n_det"] and info[s, k, 6] == ro["n_corr"], (s, k)
            assert bool(info[s, k, 7]) == ro["used_bruteforce"], (s, k)
            if ro["updated"]:
                dp, dr = pose_diff(rec["T"][s, k].reshape(4, 4), ro["T"])
                assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (s, k, dp, dr)
    n_retry = int(((info[:, 1:, 2] == seqs[0]["cols"]) & (info[:, 1:, 4] >= 1)).sum())
    n_reinit = int(info[:, 1:, 7].sum())
    assert n_retry >= 1 and n_reinit >= 1, (n_retry, n_reinit)


@pytest.mark.gpu
def test_mixed_device_sequences_equal_host_sequences():
    """5 streams of five set-ups (three cameras, 4 / 5 / 8 markers, two parameter sets) on one handle, drop-outs in two
    of them: records and info of the device-frame entries equal those of the host-frame entries as bytes."""
    kw4 = dict(threshold_value=120, gaussian_sigma=0.8, nearest_neighbour_pixel_tolerance=6.0,
               back_projection_pixel_tolerance=4.0)
    S = [("C2", None, {}), ("C2", _camera_b(), {}), ("C1", _camera_c(), {}), ("C3", None, {}), ("C2", None, kw4)]
    drop = {1: (9,), 3: (15,)}
    seqs = [synth.make_sequence(cfg, N_FRAMES, seed=1900 + j, dropout=drop.get(j, ()), camera=cam)
            for j, (cfg, cam, kw) in enumerate(S)]
    out = _run_both(seqs, [kw for _, _, kw in S])
    assert out["device"][0].tobytes() == out["host"][0].tobytes()
    assert np.array_equal(out["device"][1], out["host"][1])
    rec, info = out["device"]
    assert int((rec["status"] == 0).sum()) >= 5 * (N_FRAMES - 6)
    assert int(((info[:, 1:, 2] == seqs[0]["cols"]) & (info[:, 1:, 4] >= 1)).sum()) >= 1     # whole-image retries


@pytest.mark.gpu
def test_device_submit_refuses_host_memory_and_stays_usable():
    """A frame in pinned host memory (device-accessible on purpose: a broken check cannot fault the card, it makes this
    test fail) is refused with MPE_ERR_ARG and nothing is submitted; a second _device_submit while one is pending is
    refused; _cancel after a device submit frees the handle; and the handle gives the same records afterwards."""
    import torch
    lib = mpe.load_library()
    q = synth.make_sequence("C2", 1, seed=990)
    rows, cols = int(q["rows"]), int(q["cols"])
    img = np.ascontiguousarray(q["frames"][0])
    d_img = torch.from_numpy(img).cuda()
    pinned = mpe.PinnedFrames(1, rows, cols)
    pinned.array[0] = img
    K, D = np.ascontiguousarray(q["K"], np.float64), np.ascontiguousarray(q["D"], np.float64)
    markers = np.ascontiguousarray(q["markers"], np.float64)
    P = mpe.demo_params()
    pred = np.ascontiguousarray(synth.project(q["T_true"][0], q["markers"], q["K"]), np.float64)
    px = synth.distort_px(pred, q["K"], q["D"])
    x0, y0 = [max(0, int(v) - 40) for v in px.min(0)]
    x1, y1 = min(cols, int(px[:, 0].max()) + 40), min(rows, int(px[:, 1].max()) + 40)
    su = (mpe.binding.TrackSetup * 1)(mpe.binding.TrackSetup(ctypes.addressof(P), K.ctypes.data, D.ctypes.data, len(D),
                                                             markers.ctypes.data, len(markers)))
    h = mpe.Handle(0)
    hp = h._h
    torch.cuda.synchronize()

    def items(p0, p1, roi_x=0):
        it = (mpe.binding.TrackItem * 2)()
        it[0] = mpe.binding.TrackItem(p0, roi_x, 0, cols, rows, None)                        # whole image, detection only
        it[1] = mpe.binding.TrackItem(p1, x0, y0, x1 - x0, y1 - y0, pred.ctypes.data)        # tracked around the LEDs
        return it

    def submit(it, idx=None):
        return lib.mpe_track_step_batch_setups_device_submit(hp, it, idx, 2, rows, cols, cols, su, 1)

    def collect():
        dets, corr, res = np.zeros(2, mpe.DETECTIONS_DTYPE), np.zeros(2 * 32, np.uint32), np.zeros(2, mpe.RESULT_DTYPE)
        assert lib.mpe_track_step_batch_collect(hp, ctypes.c_void_p(dets.ctypes.data), ctypes.c_void_p(corr.ctypes.data),
                                                ctypes.c_void_p(res.ctypes.data)) == 0
        assert res["status"][1] == 0 and dets["n"][0] == 5
        return dets.tobytes() + corr.tobytes() + res.tobytes()

    def refused(rc, text):
        assert rc == -1, (rc, text)
        assert text in lib.mpe_last_error(hp).decode(), lib.mpe_last_error(hp).decode()

    d, p = d_img.data_ptr(), pinned.array.ctypes.data
    try:
        assert submit(items(d, d)) == 0
        ref = collect()
        n0 = h.get_option("track_batch_submits")
        cases = [(items(p, d), None, "the host entries are for that"),                    # pinned memory, first item
                 (items(d, p), None, "the host entries are for that"),                    # ... behind a checked allocation
                 (items(d, img.ctypes.data), None, "the host entries are for that"),      # ordinary host memory
                 (items(d, d, roi_x=1), None, "ROI outside the image"),
                 (items(d, d), (ctypes.c_int * 2)(0, 1), "set-up index out of range")]
        for it, idx, text in cases:
            refused(submit(it, idx), text)
            assert h.get_option("track_batch_submits") == n0, text
            assert submit(items(d, d)) == 0, text
            assert collect() == ref, text
            n0 += 1
        # one outstanding submission per handle, whichever entry made it
        assert submit(items(d, d)) == 0
        refused(submit(items(d, d)), "a submitted batch has not been collected yet")
        assert collect() == ref
        # _cancel after a device submit frees the handle; there is then nothing to collect
        assert submit(items(d, d)) == 0
        assert lib.mpe_track_step_batch_cancel(hp) == 0
        dets, corr, res = np.zeros(2, mpe.DETECTIONS_DTYPE), np.zeros(2 * 32, np.uint32), np.zeros(2, mpe.RESULT_DTYPE)
        assert lib.mpe_track_step_batch_collect(hp, ctypes.c_void_p(dets.ctypes.data), ctypes.c_void_p(corr.ctypes.data),
                                                ctypes.c_void_p(res.ctypes.data)) == -1
        assert submit(items(d, d)) == 0 and collect() == ref
        # the tracker entry refuses host frames as well, and leaves the handle free
        t = mpe.Tracker(h, markers, K, D, P)
        ptrs = (ctypes.c_void_p * 1)(p)
        times = np.zeros(1)
        rc = lib.mpe_tracker_estimate_batch_device((ctypes.c_void_p * 1)(t._t), 1, ptrs, rows, cols, cols,
                                                   times.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None, None)
        t.close()
        refused(rc, "the host entries are for that")
        assert submit(items(d, d)) == 0 and collect() == ref
    finally:
        lib.mpe_track_step_batch_cancel(hp)
        h.close()
        pinned.close()
