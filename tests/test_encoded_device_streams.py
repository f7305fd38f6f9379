"""Lock-step tracking of device frames in the camera's own encoding (mpe_track_step_batch_setups_device_encoded[_submit],
mpe_tracker_estimate_batch_device_encoded, mpe_tracker_run_sequences_batch_device_encoded_threads): the ROI gather decodes
the pixels it gathers (k_gather_rois_encoded), so every record must equal, byte for byte, what the mono8 device entries
return over the same frames after mpe_convert_to_mono8 — and what the host entries return over frames converted by the
oracle.  CPU tier: exports, usage errors, and the segment arithmetic compiled for the host and run under
AddressSanitizer; GPU tier: the stage entry, the tracker entries and refusals on a device."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from rpg_monocular_pose_estimator_amd import synth
import rpg_monocular_pose_estimator_amd as mpe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")
NEW_SYMBOLS = ("mpe_track_step_batch_setups_device_encoded", "mpe_track_step_batch_setups_device_encoded_submit",
               "mpe_tracker_estimate_batch_device_encoded", "mpe_tracker_run_sequences_batch_device_encoded_threads")
MPE_ERR_ARG, MPE_ERR_UNSUPPORTED = -1, -3
BPP = {"bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4, "mono16": 2}
# (encoding, big_endian): the five encodings and mono16 in both byte orders
VARIANTS = [("bgr8", False), ("rgb8", False), ("bgra8", False), ("rgba8", False), ("mono16", False), ("mono16", True)]


@pytest.fixture(scope="module")
def lib():
    mpe.build_library()
    return mpe.load_library()


# ---- CPU tier -----------------------------------------------------------------------------------------------------

def test_encoded_entries_are_exported(lib):
    import inspect
    names = mpe.exported_symbols()
    for s in NEW_SYMBOLS:
        assert s in names, s
        assert hasattr(lib, s), s
    for f in (mpe.Handle.track_step_batch_device, mpe.tracker_estimate_batch_device, mpe.tracker_run_sequences_batch_device):
        par = inspect.signature(f).parameters
        assert par["encoding"].default == "mono8" and par["big_endian"].default is False, f


def test_encoded_entries_reject_bad_usage_without_a_device(lib):
    """Null handle, null trackers, duplicates, trackers of different handles, n == 0 and n_threads < 1: refused (or
    nothing to do) before any device work, as the mono8 device-frame entries refuse them."""
    fr = np.zeros((2, 16, 48), np.uint8)     # (never read: every call is refused before it looks at a frame)
    ptrs = (ctypes.c_void_p * 2)(fr.ctypes.data, fr.ctypes.data)
    times = np.zeros(2)
    dp = times.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    null_ts = (ctypes.c_void_p * 1)(None)
    setup_idx = (ctypes.c_int * 1)(0)
    sub = lib.mpe_track_step_batch_setups_device_encoded_submit
    assert sub(None, None, setup_idx, 1, 16, 16, 48, 1, 0, None, 1) == MPE_ERR_ARG
    assert sub(None, None, None, 1, 16, 16, 48, 1, 0, None, 1) == MPE_ERR_ARG
    assert sub(None, None, None, 1, 16, 16, 48, 6, 0, None, 1) == MPE_ERR_ARG       # (the null handle comes first)
    assert lib.mpe_track_step_batch_setups_device_encoded(None, None, setup_idx, 1, 16, 16, 48, 1, 0, None, 1, None, None,
                                                          None) == MPE_ERR_ARG
    call = lib.mpe_tracker_estimate_batch_device_encoded
    assert call(None, 1, ptrs, 16, 16, 48, 1, 0, dp, None, None, None) == MPE_ERR_ARG        # no trackers
    assert call(null_ts, 1, ptrs, 16, 16, 48, 1, 0, dp, None, None, None) == MPE_ERR_ARG     # null tracker
    assert call(null_ts, 1, None, 16, 16, 48, 1, 0, dp, None, None, None) == MPE_ERR_ARG     # no frames
    assert call(null_ts, 0, ptrs, 16, 16, 48, 1, 0, dp, None, None, None) == 0               # nothing to do
    run = lib.mpe_tracker_run_sequences_batch_device_encoded_threads
    assert run(None, 1, ptrs, 2, 16, 16, 48, 768, 1, 0, dp, None, None, 2) == MPE_ERR_ARG    # no trackers
    assert run(null_ts, 1, ptrs, 2, 16, 16, 48, 768, 1, 0, dp, None, None, 2) == MPE_ERR_ARG  # null tracker
    assert run(null_ts, 1, ptrs, 2, 16, 16, 48, 768, 1, 0, dp, None, None, 0) == MPE_ERR_ARG  # n_threads < 1
    assert run(null_ts, 0, ptrs, 2, 16, 16, 48, 768, 1, 0, dp, None, None, 1) == 0           # nothing to do
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
        assert call(other, 2, ptrs, 16, 16, 48, 1, 0, dp, None, None, None) == MPE_ERR_ARG   # different handles
        assert call(dup, 2, ptrs, 16, 16, 48, 1, 0, dp, None, None, None) == MPE_ERR_ARG     # the same tracker twice
        assert run(dup, 2, ptrs, 2, 16, 16, 48, 768, 1, 0, dp, None, None, 1) == MPE_ERR_ARG  # ... twice in a group
    finally:
        for t in ts:
            lib.mpe_tracker_destroy(t)


def test_encoded_gather_arithmetic_on_the_host_under_sanitizers(tmp_path):
    """csrc/mpe_gather.h, gather_segment_encoded — what k_gather_rois_encoded computes per 16 pixels — as a stand-alone
    host program built with AddressSanitizer + UBSan: 2 000 seeded cases for each of bgr8, rgb8, bgra8, rgba8 and mono16
    in both byte orders (images 1 x 1 .. 24 x 40 pixels, stride = cols * bpp + {0, 1, 3, 16}, base 0 .. 3 bytes into a
    heap buffer that ends with the image, ROIs at every corner / whole image / widths 1 .. 17 / widths no multiple of
    16, slots larger than the ROI), every slot compared byte for byte with the program's own per-pixel conversion + zero
    fill.  A load outside the image, or an unaligned dword load, aborts the program (its checked loads, and the
    sanitizer behind the buffer)."""
    exe = str(tmp_path / "gather_encoded_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "tests", "host", "stub"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "gather_encoded_host.cpp"), "-o", exe])
    r = subprocess.run([exe, "2000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("bgr8", "rgb8", "bgra8", "rgba8", "mono16", "mono16 big-endian"):
        assert "gather_encoded_host ok: %s 2000 cases" % name in r.stdout, r.stdout


# ---- GPU tier -----------------------------------------------------------------------------------------------------

GUARD = 255
N_FRAMES = 12


def _encode(f, encoding, big_endian, seed):
    """Mono8 frames f (..., rows, cols) in `encoding`, as bytes (..., rows, cols, bytes per pixel).  Colour: B = f, G and
    R = f plus noise in [-6, 6], clipped (a B / R swap or a wrong weight changes bytes), alpha random.  mono16: f * 257
    plus noise in [-128, 128], clipped, in the given byte order."""
    rng = np.random.default_rng([seed, BPP[encoding], int(big_endian)])
    f = np.asarray(f)
    if encoding == "mono16":
        v = np.clip(f.astype(np.int64) * 257 + rng.integers(-128, 129, f.shape), 0, 65535).astype(np.uint16)
        hi, lo = (v >> 8).astype(np.uint8), (v & 255).astype(np.uint8)
        return np.ascontiguousarray(np.stack([hi, lo] if big_endian else [lo, hi], -1))
    g = np.clip(f.astype(np.int64) + rng.integers(-6, 7, f.shape), 0, 255).astype(np.uint8)
    r = np.clip(f.astype(np.int64) + rng.integers(-6, 7, f.shape), 0, 255).astype(np.uint8)
    ch = [f, g, r] if encoding in ("bgr8", "bgra8") else [r, g, f]
    if BPP[encoding] == 4:
        ch.append(rng.integers(0, 256, f.shape).astype(np.uint8))
    return np.ascontiguousarray(np.stack(ch, -1))


def _oracle_mono8(orc, raw, encoding, big_endian):
    """The oracle's cv_bridge restatement over one encoded image given as bytes (rows, cols, bytes per pixel)."""
    src = raw.view(np.uint16)[..., 0] if encoding == "mono16" else raw     # (the declared byte order: taken as it is)
    return orc.convert_to_mono8(np.ascontiguousarray(src), encoding, big_endian)


def _guarded(raw, stride, base):
    """raw (rows, cols, bpp) inside a buffer of GUARD bytes: `base` bytes in front of it, rows `stride` bytes apart, a row
    of GUARD behind.  -> the buffer"""
    rows, cols, bpp = raw.shape
    buf = np.full(base + rows * stride + stride, GUARD, np.uint8)
    np.lib.stride_tricks.as_strided(buf[base:], (rows, cols, bpp), (stride, bpp, 1))[:] = raw
    return buf


@functools.lru_cache(maxsize=None)
def _stage_case(salt):
    import test_device_frame_streams as dfs      # (the five items of the mono8 device-frame test)
    return dfs._stage_case(salt)


CASES = [(e, b, "fused") for e, b in VARIANTS] + [(e, False, v) for e in ("bgr8", "mono16") for v in ("chain", "overflow")]


@pytest.mark.gpu
@pytest.mark.parametrize("encoding,big_endian,variant", CASES,
                         ids=["%s%s-%s" % (e, "-be" if b else "", v) for e, b, v in CASES])
def test_stage_entry_equals_convert_then_device_entry_and_oracle_convert_then_host_entry(orc, encoding, big_endian, variant):
    """One time step over the five items of the mono8 device-frame test (a ROI at each image corner over two set-ups,
    one with odd roi_x and a width that is no multiple of 4, and a whole-image detection-only item), the frames
    encoded, in buffers of 255-valued guard bytes, rows cols * bpp + 3 bytes apart, the image an odd number of bytes
    into its tensor.  (a) detections, correspondences and records equal as bytes those of Handle.convert_to_mono8 on
    the device followed by track_step_batch_device; (b) and those of the host entry track_step_batch over frames
    converted by the oracle (which does not pass through k_to_mono8).  chain: track_fused 0; overflow: salt-noise
    frames, whose slots overflow the small blob tier and are re-run in _collect from the gathered (mono8) slots."""
    import torch
    c = _stage_case(0.002 if variant == "overflow" else 0.0)
    rows, cols, bpp = c["rows"], c["cols"], BPP[encoding]
    stride = cols * bpp + 3
    base = 2 * stride + 1
    raw = [_encode(f, encoding, big_endian, 77 + k) for k, f in enumerate(c["frames"])]
    ref_frames = [_oracle_mono8(orc, r, encoding, big_endian) for r in raw]
    if variant != "overflow":      # the encoded frames still show the five LEDs in every ROI asserted on below
        for i in range(4):
            markers, K, D, _ = c["setups"][c["which"][i]]
            und, _ = orc.find_leds(ref_frames[c["which"][i]], orc.make_params(), K, D, roi=c["rois"][i])
            assert len(und) == 5, (i, len(und))
    dev_bufs = [torch.from_numpy(_guarded(r, stride, base)).cuda() for r in raw]
    dev = [torch.as_strided(t, (rows, cols, bpp), (stride, bpp, 1), base) for t in dev_bufs]
    assert dev[0].data_ptr() % 2 == 1
    h = mpe.Handle(0)
    try:
        if variant == "chain":
            h.set_option("track_fused", 0)
        conv = h.convert_to_mono8(torch.stack([d.contiguous() for d in dev]), encoding, big_endian)   # (2, rows, cols)
        for k in range(2):
            assert np.array_equal(conv[k].cpu().numpy(), ref_frames[k]), k
        names = ("track_batch_submits", "track_batch_chains", "track_batch_reruns")
        out, counts = {}, {}
        for entry in ("mono8", "encoded", "host"):
            c0 = [h.get_option(k) for k in names]
            if entry == "mono8":
                r = h.track_step_batch_device([conv[w] for w in c["which"]], c["rois"], c["preds"], c["setups"], c["which"])
            elif entry == "encoded":
                r = h.track_step_batch_device([dev[w] for w in c["which"]], c["rois"], c["preds"], c["setups"], c["which"],
                                              encoding=encoding, big_endian=big_endian)
            else:
                r = h.track_step_batch([ref_frames[w] for w in c["which"]], c["rois"], c["preds"], c["setups"], c["which"])
            out[entry] = r
            counts[entry] = [h.get_option(k) - v for k, v in zip(names, c0)]
        for k, what in enumerate(("detections", "correspondences", "records")):
            assert out["encoded"][k].tobytes() == out["mono8"][k].tobytes(), what       # anchor (a)
            assert out["encoded"][k].tobytes() == out["host"][k].tobytes(), what        # anchor (b)
        assert counts["encoded"] == counts["mono8"], counts
        assert counts["encoded"][0] == 1
        dets, corr, res = out["encoded"]
        if variant == "overflow":
            assert counts["encoded"][2] >= 1, counts
        else:
            assert counts["encoded"][1] == (2 if variant == "chain" else 0), counts
            assert (res["status"][:4] == 0).all(), res["status"]            # every corner ROI was tracked to a pose
            assert (dets["n"][:4] == 5).all(), dets["n"]
    finally:
        h.close()


def _sequences():
    """3 streams of three set-ups (two cameras; 5, 5 and 4 markers), 12 frames, one drop-out frame in stream 0.  With
    seed 951 stream 0 loses its pose on frame 1 and is re-initialised by brute force on frames 1 and 2, and searches
    the whole image again on frames 2 and 5 (the drop-out) — by the oracle's state machine on the CPU."""
    import test_device_frame_streams as dfs
    S = [("C2", None, 951, (5,)), ("C2", dfs._camera_b(), 2311, ()), ("C1", None, 2302, ())]
    return [synth.make_sequence(cfg, N_FRAMES, seed=seed, dropout=drop, camera=cam) for cfg, cam, seed, drop in S]


@pytest.mark.gpu
@pytest.mark.parametrize("encoding", ["bgr8", "mono16"])
def test_encoded_sequences_equal_mono8_device_sequences(orc, encoding):
    """tracker_run_sequences_batch_device(..., encoding=...) over encoded sequences against the mono8 device entry over
    the sequences after Handle.convert_to_mono8: records and info equal as bytes; the per-step entry reproduces the
    loop's records step by step; and the run contains a whole-image retry and a brute-force re-initialisation (the
    drop-out frame), so whole frames are decoded by the gather as well.  mono16 goes in as (n, rows, cols) int16
    tensors, bgr8 as (n, rows, cols, 3) uint8."""
    import torch
    seqs = _sequences()
    times = seqs[0]["times"]
    raw = [_encode(q["frames"], encoding, False, 900 + j) for j, q in enumerate(seqs)]
    # the oracle's state machine over the oracle-converted frames: the retry and the re-initialisation are there
    q0 = seqs[0]
    to = orc.Tracker(q0["markers"], q0["K"], q0["D"], orc.make_params())
    ro = [to.estimate(_oracle_mono8(orc, raw[0][k], encoding, False), times[k]) for k in range(N_FRAMES)]
    to.close()
    assert any(r["used_bruteforce"] for r in ro[1:]) and not all(r["updated"] for r in ro)
    if encoding == "mono16":
        d_enc = [torch.from_numpy(np.ascontiguousarray(r).view(np.int16)[..., 0]).cuda() for r in raw]
    else:
        d_enc = [torch.from_numpy(r).cuda() for r in raw]
    h = mpe.Handle(0)
    made = []

    def trackers():
        ts = [mpe.Tracker(h, q["markers"], q["K"], q["D"], mpe.demo_params()) for q in seqs]
        made.extend(ts)
        return ts

    try:
        d_mono = [h.convert_to_mono8(t, encoding) for t in d_enc]
        for j in (0, 1):
            assert np.array_equal(d_mono[j][5].cpu().numpy(), _oracle_mono8(orc, raw[j][5], encoding, False)), j
        ref = mpe.tracker_run_sequences_batch_device(trackers(), d_mono, times)
        c0 = h.get_option("track_batch_submits")
        got = mpe.tracker_run_sequences_batch_device(trackers(), d_enc, times, encoding=encoding)
        assert h.get_option("track_batch_submits") - c0 >= N_FRAMES
        assert got[0].tobytes() == ref[0].tobytes()
        assert np.array_equal(got[1], ref[1])
        ts = trackers()
        for k in range(N_FRAMES):
            r, i, upd = mpe.tracker_estimate_batch_device(ts, [f[k] for f in d_enc], [times[k]] * len(seqs), encoding=encoding)
            assert r.tobytes() == got[0][:, k].tobytes() and np.array_equal(i, got[1][:, k]), k
            assert np.array_equal(upd, r["status"] == 0), k
        rec, info = got
        assert [bool(x) for x in info[0, :, 7]] == [r["used_bruteforce"] for r in ro]
        assert [bool(s == 0) for s in rec["status"][0]] == [r["updated"] for r in ro]
        n_retry = int(((info[:, 1:, 2] == seqs[0]["cols"]) & (info[:, 1:, 4] >= 1)).sum())
        n_reinit = int(info[:, 1:, 7].sum())
        assert n_retry >= 1 and n_reinit >= 1, (n_retry, n_reinit)
        assert int((rec["status"] == 0).sum()) >= 3 * (N_FRAMES - 3)
    finally:
        for t in made:
            t.close()
        h.close()


@pytest.mark.gpu
def test_encoded_submit_refusals_leave_the_handle_usable(orc):
    """On a device: a stride below cols * bpp is MPE_ERR_ARG, encoding 6 MPE_ERR_UNSUPPORTED, a frame in pinned host
    memory (device-accessible on purpose: a broken check cannot fault the card, it makes this test fail) is refused
    with "the host entries are for that"; nothing is submitted by any of them and the handle gives the reference records
    afterwards; a pending encoded submit blocks a second one; _cancel frees the handle."""
    import torch
    lib = mpe.load_library()
    q = synth.make_sequence("C2", 1, seed=990)
    rows, cols = int(q["rows"]), int(q["cols"])
    raw = _encode(q["frames"][0], "bgr8", False, 5)
    d_img = torch.from_numpy(raw).cuda()
    pinned = mpe.PinnedFrames(1, rows, cols * 3)
    pinned.array[0] = raw.reshape(rows, cols * 3)
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
    ENC_BGR8 = mpe.binding.ENCODINGS["bgr8"]

    def items(p0, p1):
        it = (mpe.binding.TrackItem * 2)()
        it[0] = mpe.binding.TrackItem(p0, 0, 0, cols, rows, None)                            # whole image, detection only
        it[1] = mpe.binding.TrackItem(p1, x0, y0, x1 - x0, y1 - y0, pred.ctypes.data)        # tracked around the LEDs
        return it

    def submit(it, stride=3 * cols, enc=ENC_BGR8):
        return lib.mpe_track_step_batch_setups_device_encoded_submit(hp, it, None, 2, rows, cols, stride, enc, 0, su, 1)

    def collect():
        dets, corr, res = np.zeros(2, mpe.DETECTIONS_DTYPE), np.zeros(2 * 32, np.uint32), np.zeros(2, mpe.RESULT_DTYPE)
        assert lib.mpe_track_step_batch_collect(hp, ctypes.c_void_p(dets.ctypes.data), ctypes.c_void_p(corr.ctypes.data),
                                                ctypes.c_void_p(res.ctypes.data)) == 0
        assert res["status"][1] == 0 and dets["n"][0] == 5
        return dets.tobytes() + corr.tobytes() + res.tobytes()

    d, p = d_img.data_ptr(), pinned.array.ctypes.data
    try:
        assert submit(items(d, d)) == 0
        ref = collect()
        # ... which are the records of the mono8 device entry over the converted frame
        mono = torch.from_numpy(_oracle_mono8(orc, raw, "bgr8", False)).cuda()
        torch.cuda.synchronize()
        assert lib.mpe_track_step_batch_setups_device_submit(hp, items(mono.data_ptr(), mono.data_ptr()), None, 2, rows, cols,
                                                             cols, su, 1) == 0
        assert collect() == ref
        n0 = h.get_option("track_batch_submits")
        cases = [(dict(it=items(d, d), stride=3 * cols - 1), MPE_ERR_ARG, "bad argument"),
                 (dict(it=items(d, d), enc=6), MPE_ERR_UNSUPPORTED, "encoding not supported"),
                 (dict(it=items(d, d), enc=-1), MPE_ERR_UNSUPPORTED, "encoding not supported"),
                 (dict(it=items(p, d)), MPE_ERR_ARG, "the host entries are for that"),        # pinned memory, first item
                 (dict(it=items(d, p)), MPE_ERR_ARG, "the host entries are for that")]        # ... behind a checked allocation
        for kw, code, text in cases:
            assert submit(**kw) == code, (code, text)
            assert text in lib.mpe_last_error(hp).decode(), lib.mpe_last_error(hp).decode()
            assert h.get_option("track_batch_submits") == n0, text
            assert submit(items(d, d)) == 0, text
            assert collect() == ref, text
            n0 += 1
        # one outstanding submission per handle, whichever entry made it
        assert submit(items(d, d)) == 0
        assert submit(items(d, d)) == MPE_ERR_ARG
        assert "a submitted batch has not been collected yet" in lib.mpe_last_error(hp).decode()
        assert collect() == ref
        # _cancel after an encoded submit frees the handle; there is then nothing to collect
        assert submit(items(d, d)) == 0
        assert lib.mpe_track_step_batch_cancel(hp) == 0
        dets, corr, res = np.zeros(2, mpe.DETECTIONS_DTYPE), np.zeros(2 * 32, np.uint32), np.zeros(2, mpe.RESULT_DTYPE)
        assert lib.mpe_track_step_batch_collect(hp, ctypes.c_void_p(dets.ctypes.data), ctypes.c_void_p(corr.ctypes.data),
                                                ctypes.c_void_p(res.ctypes.data)) == -1
        assert submit(items(d, d)) == 0 and collect() == ref
        # the tracker entry refuses an unknown encoding and host frames as well, and leaves the handle free
        t = mpe.Tracker(h, markers, K, D, P)
        times = np.zeros(1)
        tp = times.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        call = lib.mpe_tracker_estimate_batch_device_encoded
        rc_enc = call((ctypes.c_void_p * 1)(t._t), 1, (ctypes.c_void_p * 1)(d), rows, cols, 3 * cols, 6, 0, tp, None, None, None)
        rc_pin = call((ctypes.c_void_p * 1)(t._t), 1, (ctypes.c_void_p * 1)(p), rows, cols, 3 * cols, ENC_BGR8, 0, tp, None,
                      None, None)
        msg = lib.mpe_last_error(hp).decode()
        t.close()
        assert rc_enc == MPE_ERR_UNSUPPORTED and rc_pin == MPE_ERR_ARG and "the host entries are for that" in msg
        assert submit(items(d, d)) == 0 and collect() == ref
    finally:
        lib.mpe_track_step_batch_cancel(hp)
        h.close()
        pinned.close()
