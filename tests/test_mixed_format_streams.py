"""Lock-step groups of cameras that differ in image size, row stride and encoding (mpe_track_step_batch_formats[_submit],
mpe_tracker_estimate_batch_formats, mpe_tracker_run_sequences_batch_formats_threads): ONE submission per time step for a
rig that the entries with one rows / cols / stride / encoding per call need one submission per format for; every record
must equal what those entries return over the items or trackers of each format alone.  CPU tier: exports, usage errors,
and the arithmetic of k_gather_rois_formats compiled for the host and run under AddressSanitizer + UBSan; GPU tier: the
stage entry on device and on host frames, the tracker entries, and refusals on a device.

Stage-entry records are compared over what a record DEFINES: n, status and the first n points of a detection set; the
status of a result and, for a pose, its pose, covariance, counts and the first n_corr correspondence rows.  The bytes
beyond a record's valid entries are what the device buffer last held at that offset, which depends on the number of items
of the submission (tests/test_device_frame_streams.py compares a subset field by field for the same reason).  Tracker
records and info are written by the host from tracker state and are compared as bytes."""
import ctypes
import functools
import inspect
import os
import subprocess

import numpy as np
import pytest

from rpg_monocular_pose_estimator_amd import synth
import rpg_monocular_pose_estimator_amd as mpe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")
NEW_SYMBOLS = ("mpe_track_step_batch_formats", "mpe_track_step_batch_formats_submit", "mpe_tracker_estimate_batch_formats",
               "mpe_tracker_run_sequences_batch_formats_threads")
MPE_ERR_ARG, MPE_ERR_UNSUPPORTED = -1, -3
BPP = {"mono8": 1, "bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4, "mono16": 2}


@pytest.fixture(scope="module")
def lib():
    mpe.build_library()
    return mpe.load_library()


def _fmt(rows, cols, stride, encoding="mono8", big_endian=False):
    return mpe.ImageFormat(int(rows), int(cols), int(stride), mpe.ENCODINGS.get(encoding, encoding), int(big_endian))


# ---- CPU tier -----------------------------------------------------------------------------------------------------

def test_format_entries_are_exported(lib):
    names = mpe.exported_symbols()
    for s in NEW_SYMBOLS:
        assert s in names, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s          # declared in the binding
    for f in (mpe.Handle.track_step_batch_formats, mpe.tracker_estimate_batch_formats, mpe.tracker_run_sequences_batch_formats):
        assert inspect.signature(f).parameters["formats"].default is None, f
    assert inspect.signature(mpe.tracker_run_sequences_batch_formats).parameters["threads"].default == 1
    assert ctypes.sizeof(mpe.ImageFormat) == 24 and mpe.binding.ImageFormat is mpe.ImageFormat


def test_format_entries_reject_bad_usage_without_a_device(lib):
    """Null handle, null trackers / frames / formats / frame strides, duplicates, trackers of different handles,
    n_threads < 1: refused before any device work; n == 0: nothing to do."""
    fr = np.zeros((2, 16, 48), np.uint8)     # (never read: every call is refused before it looks at a frame)
    ptrs = (ctypes.c_void_p * 2)(fr.ctypes.data, fr.ctypes.data)
    times = np.zeros(2)
    dp = times.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    null_ts = (ctypes.c_void_p * 1)(None)
    fmts = (mpe.ImageFormat * 2)(_fmt(16, 16, 48, "bgr8"), _fmt(16, 48, 48))
    fstr = (ctypes.c_size_t * 2)(768, 768)
    idx = (ctypes.c_int * 1)(0)
    sub = lib.mpe_track_step_batch_formats_submit
    assert sub(None, None, idx, idx, 1, fmts, 2, 1, None, 1) == MPE_ERR_ARG                   # null handle
    assert sub(None, None, None, None, 1, None, 1, 1, None, 1) == MPE_ERR_ARG
    assert lib.mpe_track_step_batch_formats(None, None, idx, idx, 1, fmts, 2, 1, None, 1, None, None, None) == MPE_ERR_ARG
    call = lib.mpe_tracker_estimate_batch_formats
    assert call(None, 1, ptrs, 1, fmts, dp, None, None, None) == MPE_ERR_ARG                  # no trackers
    assert call(null_ts, 1, ptrs, 1, fmts, dp, None, None, None) == MPE_ERR_ARG               # null tracker
    assert call(null_ts, 1, None, 1, fmts, dp, None, None, None) == MPE_ERR_ARG               # no frames
    assert call(null_ts, 1, ptrs, 1, None, dp, None, None, None) == MPE_ERR_ARG               # no formats
    assert call(null_ts, 0, ptrs, 1, fmts, dp, None, None, None) == 0                         # nothing to do
    run = lib.mpe_tracker_run_sequences_batch_formats_threads
    assert run(None, 1, ptrs, 2, 1, fmts, fstr, dp, None, None, 2) == MPE_ERR_ARG             # no trackers
    assert run(null_ts, 1, ptrs, 2, 1, fmts, fstr, dp, None, None, 2) == MPE_ERR_ARG          # null tracker
    assert run(null_ts, 1, None, 2, 1, fmts, fstr, dp, None, None, 2) == MPE_ERR_ARG          # no frames
    assert run(null_ts, 1, ptrs, 2, 1, None, fstr, dp, None, None, 2) == MPE_ERR_ARG          # no formats
    assert run(null_ts, 1, ptrs, 2, 1, fmts, None, dp, None, None, 2) == MPE_ERR_ARG          # no frame strides
    assert run(null_ts, 1, ptrs, 2, 1, fmts, fstr, dp, None, None, 0) == MPE_ERR_ARG          # n_threads < 1
    assert run(null_ts, 0, ptrs, 2, 1, fmts, fstr, dp, None, None, 1) == 0                    # nothing to do
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
        assert call(other, 2, ptrs, 1, fmts, dp, None, None, None) == MPE_ERR_ARG             # different handles
        assert call(dup, 2, ptrs, 1, fmts, dp, None, None, None) == MPE_ERR_ARG               # the same tracker twice
        assert run(dup, 2, ptrs, 2, 1, fmts, fstr, dp, None, None, 1) == MPE_ERR_ARG          # ... twice in a group
    finally:
        for t in ts:
            lib.mpe_tracker_destroy(t)


def test_format_gather_arithmetic_on_the_host_under_sanitizers(tmp_path):
    """csrc/mpe_gather.h, gather_segment_format — what k_gather_rois_formats computes per 16 pixels — as a stand-alone
    host program built with AddressSanitizer + UBSan: 2 000 seeded cases, each a table of 2 .. 6 items whose formats are
    drawn from mono8, bgr8, rgb8, bgra8, rgba8 and mono16 in both byte orders (images 1 x 1 .. 24 x 40 pixels, stride =
    cols * bpp + {0, 1, 3, 16}, base 0 .. 3 bytes into a heap buffer of the image's own that ends with it; ROIs at every
    corner / whole image / widths 1 .. 17 / widths no multiple of 16, slots larger than the ROI; item 0's ROI at the far
    corner of an image that is smaller than item 1's), every slot compared byte for byte with the program's own per-pixel
    conversion + zero fill.  A load outside the item's own image, or an unaligned dword load, aborts the program."""
    exe = str(tmp_path / "gather_formats_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "tests", "host", "stub"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "gather_formats_host.cpp"), "-o", exe])
    r = subprocess.run([exe, "2000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gather_formats_host ok: 2000 cases" in r.stdout, r.stdout
    assert "2000 far-corner items" in r.stdout, r.stdout


# ---- GPU tier -----------------------------------------------------------------------------------------------------

N_FRAMES = 8


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


def _strided(raw, stride, channels=False):
    """raw (..., rows, cols) — channels: (..., rows, cols, bytes per pixel) — uint8 with its rows `stride` bytes apart (the
    padding 255): a view with raw's shape"""
    lead = raw.shape[:-2] if channels else raw.shape[:-1]
    row = int(np.prod(raw.shape[len(lead):]))
    buf = np.full(lead + (stride,), 255, np.uint8)
    buf[..., :row] = raw.reshape(lead + (row,))
    view = buf[..., :row].reshape(raw.shape)
    assert np.shares_memory(view, buf) and view.strides[len(lead) - 1] == stride
    return view


def _to_device(view):
    """A numpy view with padded rows as a torch CUDA tensor of the same shape and strides"""
    import torch
    base = view
    while base.base is not None:
        base = base.base
    t = torch.from_numpy(np.ascontiguousarray(base)).cuda().reshape(-1)
    return torch.as_strided(t, view.shape, view.strides, (view.ctypes.data - base.ctypes.data))


def _roi_around(q, k, cols, rows):
    pred = np.ascontiguousarray(synth.project(q["T_true"][k], q["markers"], q["K"]), np.float64)
    px = synth.distort_px(pred, q["K"], q["D"])
    x0, y0 = [max(0, int(v) - 40) for v in px.min(0)]
    x1, y1 = min(cols, int(px[:, 0].max()) + 40), min(rows, int(px[:, 1].max()) + 40)
    return (x0, y0, x1 - x0, y1 - y0), pred


def _defined(out, i):
    """What item i's records define (see the module docstring), as comparable bytes"""
    dets, corr, res = out
    n = max(int(dets["n"][i]), 0)
    parts = [dets["n"][i].tobytes(), dets["status"][i].tobytes(), dets["undist_xy"][i][:2 * n].tobytes(),
             dets["dist_xy"][i][:2 * n].tobytes(), res["status"][i].tobytes()]
    if res["status"][i] == 0:
        nc = int(res["n_corr"][i])
        parts += [res["T"][i].tobytes(), res["cov"][i].tobytes(), res["n_det"][i].tobytes(), res["n_corr"][i].tobytes(),
                  res["gn_iterations"][i].tobytes(), corr[i][:nc].tobytes()]
    return b"".join(parts)


@functools.lru_cache(maxsize=None)
def _rig():
    """Two C2 and two C4 one-frame scenes and the two set-ups (the README camera at either size)"""
    c2 = [synth.make_sequence("C2", 1, seed=s) for s in (3101, 3102)]
    c4 = [synth.make_sequence("C4", 1, seed=s) for s in (3201, 3202)]
    setups = [(q["markers"], q["K"], q["D"], mpe.demo_params()) for q in (c2[0], c4[0])]
    return c2, c4, setups


@pytest.mark.gpu
def test_stage_entry_on_device_frames_equals_the_entries_per_format():
    """Seven items of three formats in ONE call — the C2 frames as mono8 with rows cols + 5 bytes apart (format 0) and as
    bgr8 with rows 3 * cols + 3 bytes apart (format 1), the C4 frames (1920 x 1200) as big-endian mono16 (format 2) —
    with the formats interleaved (0, 2, 1, 0, 2, 1, 0), so slot order is not caller order: six tracked ROIs around the
    LEDs and one whole-image detection-only item, over two set-ups.  Every item's records equal those of
    mpe_track_step_batch_setups_device_encoded over the items of its format alone on a fresh handle; one submission."""
    c2, c4, setups = _rig()
    rows, cols, R4, C4 = 480, 752, 1200, 1920
    table = [_fmt(rows, cols, cols + 5), _fmt(rows, cols, 3 * cols + 3, "bgr8"), _fmt(R4, C4, 2 * C4, "mono16", True)]
    enc = [("mono8", False), ("bgr8", False), ("mono16", True)]
    dev = [[_to_device(_strided(q["frames"][0], cols + 5)) for q in c2],
           [_to_device(_strided(_encode(q["frames"][0], "bgr8", False, 40 + j), 3 * cols + 3, True)) for j, q in enumerate(c2)],
           [_to_device(_encode(q["frames"][0], "mono16", True, 50 + j)) for j, q in enumerate(c4)]]
    item_format = [0, 2, 1, 0, 2, 1, 0]
    which = [0, 0, 0, 1, 1, 1, 0]                      # the scene of its format that the item shows
    imgs, rois, preds, item_setup = [], [], [], []
    for i, (f, w) in enumerate(zip(item_format, which)):
        q, (r_, c_) = ((c4[w], (R4, C4)) if f == 2 else (c2[w], (rows, cols)))
        roi, pred = _roi_around(q, 0, c_, r_)
        if i == 6:
            roi, pred = (0, 0, cols, rows), None
        imgs.append(dev[f][w])
        rois.append(roi)
        preds.append(pred)
        item_setup.append(1 if f == 2 else 0)
    h = mpe.Handle(0)
    try:
        n0 = h.get_option("track_batch_submits")
        got = h.track_step_batch_formats(imgs, rois, preds, setups, item_setup, formats=table, item_format=item_format)
        assert h.get_option("track_batch_submits") - n0 == 1
    finally:
        h.close()
    dets, corr, res = got
    print("status", res["status"], "n", dets["n"])
    assert (res["status"][:6] == 0).all(), res["status"]
    assert (dets["n"][:6] == 5).all() and dets["n"][6] == 5, dets["n"]
    for f in range(3):
        a = [i for i in range(7) if item_format[i] == f]
        pick = lambda xs: [xs[i] for i in a]
        hr = mpe.Handle(0)
        try:
            ref = hr.track_step_batch_device(pick(imgs), pick(rois), pick(preds), setups, pick(item_setup), encoding=enc[f][0],
                                             big_endian=enc[f][1])
        finally:
            hr.close()
        for k, i in enumerate(a):
            assert _defined(got, i) == _defined(ref, k), (f, i)


@pytest.mark.gpu
def test_stage_entry_on_host_frames_equals_the_entry_per_format():
    """Two mono8 formats on host frames — 752 x 480 with rows 760 bytes apart, and 1920 x 1200 — four items in one call,
    against mpe_track_step_batch_setups per format; an encoded format with host frames is MPE_ERR_ARG."""
    c2, c4, setups = _rig()
    small = [_strided(q["frames"][0], 760) for q in c2]
    big = [np.ascontiguousarray(q["frames"][0]) for q in c4]
    imgs = [small[0], big[0], big[1], small[1]]
    qs = [c2[0], c4[0], c4[1], c2[1]]
    item_setup = [0, 1, 1, 0]
    rp = [_roi_around(q, 0, im.shape[1], im.shape[0]) for q, im in zip(qs, imgs)]
    rois, preds = [r for r, _ in rp], [p for _, p in rp]
    assert small[0].strides == (760, 1)
    h = mpe.Handle(0)
    try:
        n0 = h.get_option("track_batch_submits")
        got = h.track_step_batch_formats(imgs, rois, preds, setups, item_setup)
        assert h.get_option("track_batch_submits") - n0 == 1
        assert (got[2]["status"] == 0).all() and (got[0]["n"] == 5).all(), (got[2]["status"], got[0]["n"])
        for a in ([0, 3], [1, 2]):
            pick = lambda xs: [xs[i] for i in a]
            ref = h.track_step_batch(pick(imgs), pick(rois), pick(preds), setups, pick(item_setup))
            for k, i in enumerate(a):
                assert _defined(got, i) == _defined(ref, k), i
        n0 = h.get_option("track_batch_submits")
        bgr = np.zeros((480, 752, 3), np.uint8)
        with pytest.raises(mpe.MpeError, match=r"\(-1\).*host frames are mono8"):
            h.track_step_batch_formats([small[0], bgr], rois[:1] + [(0, 0, 64, 64)], preds[:1] + [None], setups, [0, 0],
                                       formats=["mono8", "bgr8"])
        assert h.get_option("track_batch_submits") == n0
    finally:
        h.close()


@functools.lru_cache(maxsize=None)
def _sequences():
    """Two C2 and two C4 sequences of 8 frames; the first C2 stream drops to two LEDs on frame 4"""
    return ([synth.make_sequence("C2", N_FRAMES, seed=951, dropout=(4,)), synth.make_sequence("C2", N_FRAMES, seed=2311)],
            [synth.make_sequence("C4", N_FRAMES, seed=4101), synth.make_sequence("C4", N_FRAMES, seed=4102)])


@pytest.mark.gpu
def test_tracker_entries_equal_the_encoded_entries_per_format():
    """One lock-step group on one handle over the four kinds of stream — C2 mono8, C2 rgba8, C4 mono8 with rows
    cols + 16 bytes apart, C4 little-endian mono16 —, two streams of each kind (so that the references below hold two
    trackers per call), 8 device frames each; the first C2 sequence drops to two LEDs on frame 4, so a whole-image retry
    and a re-initialisation happen inside the group.  Records, info and updated of every stream and step are
    byte-identical to fresh trackers run per format through mpe_tracker_estimate_batch_device_encoded; on every step
    from the third on at which no stream retried or re-initialised the group makes exactly ONE submission where the
    per-format runs make one per format; the loop in C over the same sequences returns the same records."""
    c2, c4 = _sequences()
    times = c2[0]["times"]
    kinds = [("mono8", c2, lambda f: f), ("rgba8", c2, lambda f: _encode(f, "rgba8", False, 61)),
             ("mono8", c4, lambda f: _strided(f, 1920 + 16)), ("mono16", c4, lambda f: _encode(f, "mono16", False, 62))]
    seqs, d_seq, spec = [], [], []          # format-major: streams 2 k and 2 k + 1 are of kind k
    for name, qs, conv in kinds:
        for q in qs:
            seqs.append(q)
            d_seq.append(_to_device(conv(q["frames"])))
            spec.append(name)
    N = len(seqs)
    assert d_seq[4].stride(1) == 1936 and d_seq[2].shape == (N_FRAMES, 480, 752, 4)
    h = mpe.Handle(0)
    made = []

    def trackers(idx=range(N)):
        ts = [mpe.Tracker(h, seqs[i]["markers"], seqs[i]["K"], seqs[i]["D"], mpe.demo_params()) for i in idx]
        made.extend(ts)
        return ts

    try:
        # the group, step by step
        ts = trackers()
        rec, info, upd, sub = [], [], [], []
        for k in range(N_FRAMES):
            n0 = h.get_option("track_batch_submits")
            r, i, u = mpe.tracker_estimate_batch_formats(ts, [s[k] for s in d_seq], [times[k]] * N, formats=spec)
            sub.append(h.get_option("track_batch_submits") - n0)
            rec.append(r), info.append(i), upd.append(u)
        # per format, two fresh trackers per call, through the encoded entry
        ref_sub = np.zeros(N_FRAMES, int)
        for f in range(4):
            idx = [2 * f, 2 * f + 1]
            tf = trackers(idx)
            for k in range(N_FRAMES):
                keep, ptrs, (rows, cols), (stride, _) = mpe.binding._device_images([d_seq[i][k] for i in idx], 0, spec[idx[0]])
                n0 = h.get_option("track_batch_submits")
                r, i, u = mpe.binding._estimate_batch("mpe_tracker_estimate_batch_device_encoded", tf, ptrs, rows, cols, stride,
                                                      [times[k]] * 2, mpe.binding._enc_args(spec[idx[0]], False))
                ref_sub[k] += h.get_option("track_batch_submits") - n0
                assert r.tobytes() == rec[k][idx].tobytes(), (f, k)
                assert np.array_equal(i, info[k][idx]) and np.array_equal(u, upd[k][idx]), (f, k)
        info = np.stack(info, 1)                                    # (N, frames, 8)
        whole = np.array([[q["cols"], q["rows"]] for q in seqs])
        retried = (info[:, :, 2:4] == whole[:, None, :]).all(-1)
        steady = [k for k in range(2, N_FRAMES) if (info[:, k, 7] == 0).all() and (info[:, k - 1, 4] >= 1).all()
                  and not retried[:, k].any()]
        print("submissions per step", sub, "per-format runs", ref_sub.tolist(), "steady steps", steady)
        assert len(steady) >= 3 and len(steady) < N_FRAMES - 2, steady       # the drop-out frame is not among them
        assert info[0, 1:, 7].sum() >= 1 and retried[0, 1:].any()           # a re-initialisation and a retry happened
        assert [sub[k] for k in steady] == [1] * len(steady), sub
        assert [ref_sub[k] for k in steady] == [4] * len(steady), ref_sub
        rec = np.stack(rec, 1)
        assert int((rec["status"] == 0).sum()) >= N * (N_FRAMES - 3)
        # the loop in C, every stream with its own frame stride
        got = mpe.tracker_run_sequences_batch_formats(trackers(), d_seq, times, formats=spec)
        assert got[0].tobytes() == rec.tobytes() and np.array_equal(got[1], info)
    finally:
        for t in made:
            t.close()
        h.close()


@pytest.mark.gpu
def test_format_submit_refusals_leave_the_handle_usable():
    """On a device, each refused before anything is submitted: a ROI inside the 1920 x 1200 format of the call on an item
    of the 752 x 480 format; a format index == n_formats; a bgr8 stride of 3 * cols - 1; encodings 6 and -1; a 752 x 480
    buffer declared 1920 x 1200; pinned host memory.  Wherever a broken check would let the gather run, the item points
    into the large buffer or its ROI stays inside the small one, so that a miss fails this test and not the card.  Every
    refusal leaves the submission count unchanged and is followed by a good submit with the reference bytes; a pending
    submit blocks a second one; _cancel frees the handle."""
    import torch
    lib = mpe.load_library()
    c2, c4, setups = _rig()
    rows, cols, R4, C4 = 480, 752, 1200, 1920
    d_small = torch.from_numpy(c2[0]["frames"][0]).cuda()
    d_big = torch.from_numpy(c4[0]["frames"][0]).cuda()
    pinned = mpe.PinnedFrames(1, rows, cols)
    pinned.array[0] = c2[0]["frames"][0]
    torch.cuda.synchronize()
    keep = []
    su = (mpe.binding.TrackSetup * 2)()
    for s, (markers, K, D, P) in enumerate(setups):
        markers, K, D = [np.ascontiguousarray(v, np.float64) for v in (markers, K, D)]
        keep += [markers, K, D, P]
        su[s] = mpe.binding.TrackSetup(ctypes.addressof(P), K.ctypes.data, D.ctypes.data, len(D), markers.ctypes.data, len(markers))
    (roi_s, pred_s), (roi_b, pred_b) = _roi_around(c2[0], 0, cols, rows), _roi_around(c4[0], 0, C4, R4)
    good = (mpe.ImageFormat * 2)(_fmt(rows, cols, cols), _fmt(R4, C4, C4))
    s_, b_, p_ = d_small.data_ptr(), d_big.data_ptr(), pinned.array.ctypes.data
    h = mpe.Handle(0)
    hp = h._h

    def submit(ptrs=(s_, s_, b_), ifmt=(0, 0, 1), table=good, roi1=roi_s, roi2=roi_b):
        it = (mpe.binding.TrackItem * 3)()
        it[0] = mpe.binding.TrackItem(ptrs[0], 0, 0, cols, rows, None)              # whole small image, detection only
        it[1] = mpe.binding.TrackItem(ptrs[1], *roi1, pred_s.ctypes.data)           # tracked around the LEDs
        it[2] = mpe.binding.TrackItem(ptrs[2], *roi2, pred_b.ctypes.data)          # ... of the large image
        return lib.mpe_track_step_batch_formats_submit(hp, it, (ctypes.c_int * 3)(0, 0, 1), (ctypes.c_int * 3)(*ifmt), 3, table,
                                                       len(table), 1, su, 2)

    def collect(code=0):
        dets, corr, res = np.zeros(3, mpe.DETECTIONS_DTYPE), np.zeros((3, 16, 2), np.uint32), np.zeros(3, mpe.RESULT_DTYPE)
        assert lib.mpe_track_step_batch_collect(hp, ctypes.c_void_p(dets.ctypes.data), ctypes.c_void_p(corr.ctypes.data),
                                                ctypes.c_void_p(res.ctypes.data)) == code
        if code == 0:
            assert res["status"][1] == 0 and res["status"][2] == 0 and dets["n"][0] == 5, (res["status"], dets["n"])
        return dets.tobytes() + corr.tobytes() + res.tobytes(), (dets, corr, res)

    def table(f0=None, f1=None):
        return (mpe.ImageFormat * 2)(f0 or good[0], f1 or good[1])

    try:
        assert submit() == 0
        ref, out = collect()
        # ... which are the records of the encoded entry per format
        one = h.track_step_batch_device([d_small, d_small], [(0, 0, cols, rows), roi_s], [None, pred_s], setups[:1])
        two = h.track_step_batch_device([d_big], [roi_b], [pred_b], setups[1:])
        assert [_defined(out, i) for i in range(3)] == [_defined(one, 0), _defined(one, 1), _defined(two, 0)]
        assert submit() == 0        # (the reference again: the bytes beyond a record's valid entries are what the device
        ref, _ = collect()          #  buffer last held, and the two calls above had other shapes)
        n0 = h.get_option("track_batch_submits")
        cases = [(dict(ptrs=(s_, b_, b_), roi1=(800, 500, 100, 100)), MPE_ERR_ARG, "ROI outside the image"),
                 (dict(ifmt=(0, 2, 1)), MPE_ERR_ARG, "format index out of range"),
                 (dict(ptrs=(b_, b_, b_), table=table(f0=_fmt(rows, cols, 3 * cols - 1, "bgr8"))), MPE_ERR_ARG, "bad argument"),
                 (dict(ptrs=(b_, b_, b_), table=table(f0=_fmt(rows, cols, cols, 6))), MPE_ERR_UNSUPPORTED, "encoding not supported"),
                 (dict(ptrs=(b_, b_, b_), table=table(f0=_fmt(rows, cols, cols, -1))), MPE_ERR_UNSUPPORTED, "encoding not supported"),
                 # (the 752 x 480 buffer declared 1920 x 1200: 2.3 MB from a tensor of 0.36 MB, which the allocator keeps
                 #  in a block of 2 MB; the ROI of that item stays inside the bytes the buffer has)
                 (dict(ptrs=(s_, s_, s_), roi2=(0, 0, 64, 64)), MPE_ERR_ARG, "reaches beyond its device allocation"),
                 (dict(ptrs=(p_, s_, b_)), MPE_ERR_ARG, "the host entries are for that"),
                 (dict(ptrs=(s_, p_, b_)), MPE_ERR_ARG, "the host entries are for that")]
        for kw, code, text in cases:
            rc = submit(**kw)
            msg = lib.mpe_last_error(hp).decode()
            assert rc == code and text in msg, (rc, code, text, msg)
            assert h.get_option("track_batch_submits") == n0, text
            assert submit() == 0, text
            assert collect()[0] == ref, text
            n0 += 1
        # one outstanding submission per handle, whichever entry made it
        assert submit() == 0
        assert submit() == MPE_ERR_ARG
        assert "a submitted batch has not been collected yet" in lib.mpe_last_error(hp).decode()
        assert collect()[0] == ref
        # _cancel frees the handle; there is then nothing to collect
        assert submit() == 0
        assert lib.mpe_track_step_batch_cancel(hp) == 0
        collect(code=-1)
        assert submit() == 0 and collect()[0] == ref
        # the tracker entry refuses a bad format before it touches a tracker, and leaves the handle free
        t = mpe.Tracker(h, *setups[0][:3], setups[0][3])
        tp = np.zeros(1).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        call = lib.mpe_tracker_estimate_batch_formats
        one_t, one_p = (ctypes.c_void_p * 1)(t._t), (ctypes.c_void_p * 1)(s_)
        rc_enc = call(one_t, 1, one_p, 1, (mpe.ImageFormat * 1)(_fmt(rows, cols, cols, 6)), tp, None, None, None)
        rc_host = call(one_t, 1, one_p, 0, (mpe.ImageFormat * 1)(_fmt(rows, cols, 3 * cols, "bgr8")), tp, None, None, None)
        rc_pin = call(one_t, 1, (ctypes.c_void_p * 1)(p_), 1, (mpe.ImageFormat * 1)(good[0]), tp, None, None, None)
        msg = lib.mpe_last_error(hp).decode()
        t.close()
        assert (rc_enc, rc_host, rc_pin) == (MPE_ERR_UNSUPPORTED, MPE_ERR_ARG, MPE_ERR_ARG), (rc_enc, rc_host, rc_pin)
        assert "the host entries are for that" in msg
        assert submit() == 0 and collect()[0] == ref
    finally:
        lib.mpe_track_step_batch_cancel(hp)
        h.close()
        pinned.close()
