"""Bayer and YUV 4:2:2 camera frames decoded on the device (MPE_ENC_BAYER_RGGB8 .. MPE_ENC_YUV422_YUY2 = 16 .. 21):
mpe_convert_to_mono8 (k_to_mono8_bayer and the Y-byte branch of k_to_mono8), the encoded lock-step entries
(k_gather_rois_bayer, k_gather_rois_yuv), the format-table entry (k_gather_rois_formats), the wide entry and the tracker
entries.  The reference for the bytes is tests/witness_sensor_encodings.py, a numpy restatement of the rule of
include/mpe.h that nothing reference-held pins (see its docstring); everything behind the decode is compared with the
mono8 entries over the converted frames, byte for byte.

CPU tier: constants, the witness (two forms, known answers), usage errors that need no device, the segment arithmetic
compiled for the host under AddressSanitizer, the facade's frame paths.  A handle cannot exist without a device, so the
refusals that need one (stride below cols * bytes per pixel, encodings 6, 15, 22 and -1 through the entries) are in the
GPU tier; the CPU tier checks the function every entry classifies its `encoding` with for the codes -2 .. 24."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from rpg_monocular_pose_estimator_amd import synth
import rpg_monocular_pose_estimator_amd as mpe
import witness_sensor_encodings as wit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")
MPE_ERR_ARG, MPE_ERR_UNSUPPORTED = -1, -3
CODES = {"bayer_rggb8": 16, "bayer_bggr8": 17, "bayer_gbrg8": 18, "bayer_grbg8": 19, "yuv422": 20, "yuv422_yuy2": 21}
SIX = tuple(CODES)
GUARD = 255
N_FRAMES = 12


@pytest.fixture(scope="module")
def lib():
    mpe.build_library()
    return mpe.load_library()


# ---- CPU tier -----------------------------------------------------------------------------------------------------

def test_the_six_constants_are_in_the_header_and_in_the_binding():
    hdr = open(os.path.join(ROOT, "include", "mpe.h")).read()
    for name, code in CODES.items():
        m = re.search(r"#define MPE_ENC_%s\s+(\d+)\b" % name.upper(), hdr)
        assert m and int(m.group(1)) == code, name
        assert mpe.ENCODINGS[name] == code and mpe.binding.ENCODINGS[name] == code, name
    for name, code in (("mono8", 0), ("bgr8", 1), ("rgb8", 2), ("bgra8", 3), ("rgba8", 4), ("mono16", 5)):
        assert mpe.ENCODINGS[name] == code, name                     # (the six existing ones keep their values)
    assert sorted(mpe.ENCODINGS.values()) == list(range(6)) + list(range(16, 22))
    assert "are not covered" not in hdr and "outside the six" not in hdr


def test_witness_forms_agree_and_give_the_known_answers():
    """The literal loop and the colour-map form on all sizes 1 x 1 .. 8 x 8 and all four patterns; the hand-checked known
    answers (the first one: ((7 + 209 + 81 + 239) * 4899 + (108 + 44 + 96 + 32) * 9617 + 198 * 4 * 1868 +
    32768) >> 16 = 104); a constant image; YUV picks the Y byte."""
    assert ((7 + 209 + 81 + 239) * 4899 + (108 + 44 + 96 + 32) * 9617 + 198 * 4 * 1868 + 32768) >> 16 == 104
    rng = np.random.default_rng(20)
    for enc in wit.BAYER:
        for rows in range(1, 9):
            for cols in range(1, 9):
                img = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
                a, b = wit.bayer_to_gray_loop(img, enc), wit.bayer_to_gray(img, enc)
                assert np.array_equal(a, b), (enc, rows, cols)
                if rows < 3 or cols < 3:
                    assert not a.any()
        out = wit.bayer_to_gray(wit.KAT_IMAGE, enc)
        assert out[1:3, 1:4].tolist() == wit.KAT_INTERIOR[enc], (enc, out)
        assert np.array_equal(out[0], out[1]) and np.array_equal(out[3], out[2])
        assert np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, 4], out[:, 3])
        assert (wit.bayer_to_gray(np.full((5, 7), 200, np.uint8), enc) == 200).all()
        batch = rng.integers(0, 256, (3, 6, 7)).astype(np.uint8)
        assert np.array_equal(wit.bayer_to_gray(batch, enc)[2], wit.bayer_to_gray_loop(batch[2], enc))
    raw = rng.integers(0, 256, (4, 5, 2)).astype(np.uint8)        # odd cols are legal
    assert np.array_equal(wit.to_mono8(raw, "yuv422"), raw[..., 1]) and np.array_equal(wit.to_mono8(raw, "yuv422_yuy2"), raw[..., 0])


def test_new_codes_are_usage_errors_without_a_handle(lib):
    """The null handle comes first, whatever the encoding: no entry looks at a frame."""
    fr = np.zeros((2, 16, 48), np.uint8)
    ptrs = (ctypes.c_void_p * 2)(fr.ctypes.data, fr.ctypes.data)
    idx = (ctypes.c_int * 1)(0)
    for code in list(CODES.values()) + [6, 15, 22, -1]:
        assert lib.mpe_convert_to_mono8(None, ctypes.c_void_p(fr.ctypes.data), 0, code, 0, 1, 16, 16, 16, 256,
                                        ctypes.c_void_p(fr.ctypes.data), 0) == MPE_ERR_ARG
        assert lib.mpe_track_step_batch_setups_device_encoded_submit(None, None, idx, 1, 16, 16, 48, code, 0, None, 1) == MPE_ERR_ARG
        fmts = (mpe.ImageFormat * 2)(mpe.ImageFormat(16, 16, 48, code, 0), mpe.ImageFormat(16, 48, 48, 0, 0))
        assert lib.mpe_track_step_batch_formats_submit(None, None, idx, idx, 1, fmts, 2, 1, None, 1) == MPE_ERR_ARG
        assert lib.mpe_track_step_batch_wide(None, None, idx, 1, 16, 16, ctypes.c_size_t(7), 1, code, 0, None, 1, None, None,
                                             None) == MPE_ERR_ARG
    null_ts = (ctypes.c_void_p * 1)(None)
    times = np.zeros(2)
    dp = times.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.mpe_tracker_estimate_batch_device_encoded(null_ts, 1, ptrs, 16, 16, 15, 20, 0, dp, None, None, None) == MPE_ERR_ARG
    # the binding refuses an encoding it does not know, and frames of the wrong shape, before it asks the library
    with pytest.raises(mpe.MpeError):
        mpe.binding._image_format(np.zeros((4, 6, 2), np.uint8), 0, "bayer_rggb8")
    with pytest.raises(mpe.MpeError):
        mpe.binding._image_format(np.zeros((4, 6), np.uint8), 0, "yuv422")
    with pytest.raises(mpe.MpeError):
        mpe.binding._image_format(np.zeros((4, 6), np.uint16), 0, "yuv422")
    f, _, _ = mpe.binding._image_format(np.zeros((4, 6, 2), np.uint8), 0, "yuv422_yuy2")
    assert (f.rows, f.cols, f.stride_bytes, f.encoding) == (4, 6, 12, 21)
    f, _, _ = mpe.binding._image_format(np.zeros((4, 6), np.uint8), 0, "bayer_gbrg8")
    assert (f.rows, f.cols, f.stride_bytes, f.encoding) == (4, 6, 6, 18)


def test_sensor_gather_arithmetic_on_the_host_under_sanitizers(tmp_path):
    """csrc/mpe_gather.h, gather_segment_bayer and gather_segment_yuv — what k_gather_rois_bayer / _yuv compute per 16
    pixels — and gather_segment_format over tables that mix mono8, bgr8, Bayer and YUV entries, as a stand-alone host
    program built with AddressSanitizer + UBSan: 2 000 seeded cases per encoding (images 1 x 1 .. 24 x 40, so below
    3 x 3 too; stride = cols * bpp + {0, 1, 3, 16}; base 0 .. 3 bytes into a heap buffer that ends with the image; ROIs at
    every corner, the whole image, odd and even origins, widths 1 .. 17; slots larger than the ROI), every slot compared
    with the program's own per-pixel decode of the whole image plus zero fill.  A load outside the image, or an
    unaligned dword load, aborts the program.  This is the only sanitizer run of the feature."""
    exe = str(tmp_path / "gather_sensor_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "tests", "host", "stub"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "gather_sensor_host.cpp"), "-o", exe])
    r = subprocess.run([exe, "2000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gather_sensor_host ok: encodings -2 .. 24" in r.stdout, r.stdout
    for name in SIX:
        assert "gather_sensor_host ok: %s 2000 cases" % name in r.stdout, r.stdout
    assert "gather_sensor_host ok: formats 2000 cases" in r.stdout, r.stdout


def test_facade_frame_paths_with_and_without_the_opt_in():
    """framePathForEncoding: the two-argument form is what it was (Bayer and YUV through cv_bridge in both builds); the
    third argument sends yuv422 / yuv422_yuy2 (bit 0) and the Bayer patterns (bit 1) to the back-end with their own
    MPE_ENC_* code, and changes nothing else.  The glue passes the opt-in under its two build switches."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compat"), "facade_selftest"])
    exe = os.path.join(ROOT, "compat", "facade_selftest")
    names = ["mono8", "8UC1", "mono16", "bgr8", "rgba8", "16UC1", "nonsense", "bayer_rggb16"] + list(SIX)
    feed = "\n".join(names) + "\n"
    old = subprocess.run([exe, "framepath"], input=feed, capture_output=True, text=True, check=True).stdout
    got = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in old.strip().splitlines()}
    IN_PLACE, BACKEND, CV_BRIDGE = 0, 1, 2
    assert got["mono8"] == [IN_PLACE, -1, IN_PLACE, -1] and got["mono16"] == [BACKEND, 5, BACKEND, 5]
    assert got["bgr8"] == [CV_BRIDGE, -1, BACKEND, 1] and got["rgba8"] == [CV_BRIDGE, -1, BACKEND, 4]
    for n in list(SIX) + ["16UC1", "nonsense", "bayer_rggb16"]:
        assert got[n] == [CV_BRIDGE, -1, CV_BRIDGE, -1], (n, got[n])
    new = subprocess.run([exe, "framepath-sensor"], input=feed, capture_output=True, text=True, check=True).stdout
    got3 = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in new.strip().splitlines()}
    for n in names:
        per_opt = [got3[n][2 * k:2 * k + 2] for k in range(4)]        # opt-in 0, YUV, Bayer, both
        assert per_opt[0] == got[n][:2], n                            # no opt-in: the two-argument answer
        if n in CODES:
            yuv = n.startswith("yuv")
            on = [BACKEND, CODES[n]]
            assert per_opt[1] == (on if yuv else [CV_BRIDGE, -1]), (n, per_opt)
            assert per_opt[2] == ([CV_BRIDGE, -1] if yuv else on), (n, per_opt)
            assert per_opt[3] == on, (n, per_opt)
        else:
            assert per_opt[1] == per_opt[2] == per_opt[3] == per_opt[0], (n, per_opt)
    glue = open(os.path.join(ROOT, "compat", "ros", "mpe_ros_glue.cpp")).read()
    assert "MPE_BACKEND_YUV422" in glue and "MPE_OPENCV_BAYER_SCALAR" in glue and "&enc, optin)" in glue


# ---- GPU tier -----------------------------------------------------------------------------------------------------

def _bpp(encoding):
    return wit.BPP[encoding]


def _px_shape(shape, encoding):
    return tuple(shape) + ((2,) if _bpp(encoding) == 2 else ())


def _guarded_batch(raw, encoding, base, row_pad, frame_pad):
    """raw (n, rows, cols[, 2]) in a buffer of GUARD bytes: `base` bytes in front, rows cols * bpp + row_pad bytes apart,
    frames rows * stride + frame_pad apart, guard bytes behind.  -> (buffer, shape, strides in bytes)"""
    n, rows, cols = raw.shape[:3]
    bpp = _bpp(encoding)
    stride = cols * bpp + row_pad
    fstride = rows * stride + frame_pad
    buf = np.full(base + n * fstride + stride, GUARD, np.uint8)
    strides = (fstride, stride) + ((2, 1) if bpp == 2 else (1,))
    np.lib.stride_tricks.as_strided(buf[base:], raw.shape, strides)[:] = raw
    return buf, raw.shape, strides


@pytest.mark.gpu
@pytest.mark.parametrize("encoding", SIX)
def test_convert_to_mono8_equals_the_witness(hip, encoding):
    """Frames of 1 x 1, 2 x 7, 7 x 2, 3 x 3, 5 x 8, 6 x 7 and 33 x 65 in batches of 3 (a kernel that reads the
    neighbouring frame of the batch shows), from host memory, from packed device memory, and from device buffers of
    255-valued guard bytes between rows and frames with the first frame 1 byte into its tensor; one 752 x 480 frame;
    the known answers.  Byte for byte."""
    import torch
    rng = np.random.default_rng([31, CODES[encoding]])
    for rows, cols in ((1, 1), (2, 7), (7, 2), (3, 3), (5, 8), (6, 7), (33, 65)):
        raw = rng.integers(0, 256, _px_shape((3, rows, cols), encoding)).astype(np.uint8)
        ref = wit.to_mono8(raw, encoding)
        assert np.array_equal(hip.convert_to_mono8(raw, encoding), ref), (rows, cols, "host")
        assert np.array_equal(hip.convert_to_mono8(torch.from_numpy(raw).cuda(), encoding).cpu().numpy(), ref), (rows, cols)
        buf, shape, strides = _guarded_batch(raw, encoding, 1, 3, 7)
        dev = torch.as_strided(torch.from_numpy(buf).cuda(), shape, strides, 1)
        assert dev.data_ptr() % 2 == 1
        got = hip.convert_to_mono8(dev, encoding).cpu().numpy()
        assert np.array_equal(got, ref), (rows, cols, "strided", got, ref)
    raw = rng.integers(0, 256, _px_shape((1, 480, 752), encoding)).astype(np.uint8)
    assert np.array_equal(hip.convert_to_mono8(torch.from_numpy(raw).cuda(), encoding).cpu().numpy(), wit.to_mono8(raw, encoding))
    if encoding in wit.BAYER:
        out = hip.convert_to_mono8(torch.from_numpy(wit.KAT_IMAGE[None]).cuda(), encoding).cpu().numpy()[0]
        assert out[1:3, 1:4].tolist() == wit.KAT_INTERIOR[encoding], out
        flat = hip.convert_to_mono8(np.full((1, 9, 11), 200, np.uint8), encoding)
        assert (flat == 200).all()


@functools.lru_cache(maxsize=None)
def _stage_case():
    import test_device_frame_streams as dfs      # (the five items of the mono8 device-frame test)
    return dfs._stage_case(0.0)


def _guarded(raw, encoding, stride, base):
    """One frame (rows, cols[, 2]) in a buffer of GUARD bytes, `base` bytes in front, rows `stride` bytes apart, a row of
    GUARD behind.  -> (buffer, shape, strides)"""
    rows = raw.shape[0]
    buf = np.full(base + rows * stride + stride, GUARD, np.uint8)
    strides = (stride,) + ((2, 1) if _bpp(encoding) == 2 else (1,))
    np.lib.stride_tricks.as_strided(buf[base:], raw.shape, strides)[:] = raw
    return buf, raw.shape, strides


@pytest.mark.gpu
@pytest.mark.parametrize("encoding", ["bayer_rggb8", "bayer_grbg8", "yuv422", "yuv422_yuy2"])
def test_stage_entry_equals_convert_then_device_entry_and_witness_then_host_entry(orc, encoding):
    """One time step over the five items of the mono8 device-frame test (a ROI at each image corner over two set-ups,
    with odd roi_x and a width that is no multiple of 4, and a whole-image detection-only item).  The frames are
    mosaicked — every site the frame's gray value plus seeded noise in [-6, 6] — and sit in buffers of 255-valued guard
    bytes, rows cols * bpp + 3 bytes apart, the image an odd number of bytes into its tensor.  (a) detections,
    correspondences and records equal as bytes those of Handle.convert_to_mono8 on the device followed by
    track_step_batch_device; (b) and those of the host entry track_step_batch over witness-decoded frames."""
    import torch
    c = _stage_case()
    rows, cols, bpp = c["rows"], c["cols"], _bpp(encoding)
    stride = cols * bpp + 3
    base = 2 * stride + 1
    raw = [wit.mosaic(f, encoding, 77 + k) for k, f in enumerate(c["frames"])]
    ref_frames = [wit.to_mono8(r, encoding) for r in raw]
    for i in range(4):      # on the reference's side: the mosaicked frames still show the five LEDs in every corner ROI
        markers, K, D, _ = c["setups"][c["which"][i]]
        und, _ = orc.find_leds(ref_frames[c["which"][i]], orc.make_params(), K, D, roi=c["rois"][i])
        assert len(und) == 5, (i, len(und))
    dev = []
    for r in raw:
        buf, shape, strides = _guarded(r, encoding, stride, base)
        dev.append(torch.as_strided(torch.from_numpy(buf).cuda(), shape, strides, base))
    assert dev[0].data_ptr() % 2 == 1
    h = mpe.Handle(0)
    try:
        conv = h.convert_to_mono8(torch.stack([d.contiguous() for d in dev]), encoding)   # (2, rows, cols)
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
                                              encoding=encoding)
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
        assert (res["status"][:4] == 0).all(), res["status"]
        assert (dets["n"][:4] == 5).all(), dets["n"]
    finally:
        h.close()


@pytest.mark.gpu
def test_formats_entry_with_bayer_and_yuv_cameras_equals_the_entries_per_format():
    """Eight items of four formats in ONE call — the C2 frames (752 x 480) as mono8 with rows cols + 5 bytes apart, as
    bgr8 and as bayer_grbg8 with rows cols + 3 bytes apart, the C4 frames (1920 x 1200) as yuv422_yuy2 — interleaved, over
    two set-ups: seven tracked ROIs around the LEDs and one whole-image detection-only Bayer item.  Every item's records
    equal those of the single-format entry over the items of its format alone on a fresh handle; one submission."""
    import test_mixed_format_streams as mfs
    c2, c4, setups = mfs._rig()
    rows, cols, R4, C4 = 480, 752, 1200, 1920
    table = [mfs._fmt(rows, cols, cols + 5), mfs._fmt(rows, cols, 3 * cols + 3, "bgr8"),
             mfs._fmt(rows, cols, cols + 3, CODES["bayer_grbg8"]), mfs._fmt(R4, C4, 2 * C4, CODES["yuv422_yuy2"])]
    enc = ["mono8", "bgr8", "bayer_grbg8", "yuv422_yuy2"]
    dev = [[mfs._to_device(mfs._strided(q["frames"][0], cols + 5)) for q in c2],
           [mfs._to_device(mfs._strided(mfs._encode(q["frames"][0], "bgr8", False, 40 + j), 3 * cols + 3, True))
            for j, q in enumerate(c2)],
           [mfs._to_device(mfs._strided(wit.mosaic(q["frames"][0], "bayer_grbg8", 60 + j), cols + 3)) for j, q in enumerate(c2)],
           [mfs._to_device(wit.mosaic(q["frames"][0], "yuv422_yuy2", 70 + j)) for j, q in enumerate(c4)]]
    item_format = [0, 3, 2, 1, 3, 2, 0, 2]
    which = [0, 0, 0, 0, 1, 1, 1, 0]                   # the scene of its format that the item shows
    imgs, rois, preds, item_setup = [], [], [], []
    for i, (f, w) in enumerate(zip(item_format, which)):
        q, (r_, c_) = ((c4[w], (R4, C4)) if f == 3 else (c2[w], (rows, cols)))
        roi, pred = mfs._roi_around(q, 0, c_, r_)
        if i == 7:
            roi, pred = (0, 0, cols, rows), None
        imgs.append(dev[f][w])
        rois.append(roi)
        preds.append(pred)
        item_setup.append(1 if f == 3 else 0)
    h = mpe.Handle(0)
    try:
        n0 = h.get_option("track_batch_submits")
        got = h.track_step_batch_formats(imgs, rois, preds, setups, item_setup, formats=table, item_format=item_format)
        assert h.get_option("track_batch_submits") - n0 == 1
    finally:
        h.close()
    dets, corr, res = got
    print("status", res["status"], "n", dets["n"])
    assert (res["status"][:7] == 0).all(), res["status"]
    assert (dets["n"] == 5).all(), dets["n"]
    for f in range(4):
        a = [i for i in range(8) if item_format[i] == f]
        pick = lambda xs: [xs[i] for i in a]
        hr = mpe.Handle(0)
        try:
            ref = hr.track_step_batch_device(pick(imgs), pick(rois), pick(preds), setups, pick(item_setup), encoding=enc[f])
        finally:
            hr.close()
        for k, i in enumerate(a):
            assert mfs._defined(got, i) == mfs._defined(ref, k), (f, i)


SEQ_SEEDS = (951, 2311, 2302)


@functools.lru_cache(maxsize=None)
def _sequences():
    """3 streams of three set-ups (two cameras; 5, 5 and 4 markers), 12 frames, one drop-out frame in stream 0: the
    streams of test_encoded_device_streams."""
    import test_device_frame_streams as dfs
    S = [("C2", None, SEQ_SEEDS[0], (5,)), ("C2", dfs._camera_b(), SEQ_SEEDS[1], ()), ("C1", None, SEQ_SEEDS[2], ())]
    return [synth.make_sequence(cfg, N_FRAMES, seed=seed, dropout=drop, camera=cam) for cfg, cam, seed, drop in S]


@pytest.mark.gpu
@pytest.mark.parametrize("encoding", ["bayer_rggb8", "yuv422"])
def test_sensor_sequences_equal_mono8_device_sequences(orc, encoding):
    """tracker_run_sequences_batch_device(..., encoding=...) over mosaicked sequences against the mono8 device entry
    over the sequences after Handle.convert_to_mono8: records and info equal as bytes; the per-step entry reproduces
    the loop step by step; the oracle's Tracker over the witness-decoded frames of stream 0 gives the same updated /
    used_bruteforce columns.  On the oracle's side: stream 0 is re-initialised by brute force after frame 0, loses its
    pose on the drop-out, has >= 9 poses; camera b's stream >= 9; the 4-marker stream all 12."""
    import torch
    seqs = _sequences()
    times = seqs[0]["times"]
    raw = [wit.mosaic(q["frames"], encoding, 900 + j) for j, q in enumerate(seqs)]
    ro = []
    for j, q in enumerate(seqs):
        to = orc.Tracker(q["markers"], q["K"], q["D"], orc.make_params())
        ro.append([to.estimate(wit.to_mono8(raw[j][k], encoding), times[k]) for k in range(N_FRAMES)])
        to.close()
    poses = [sum(bool(r["updated"]) for r in rs) for rs in ro]
    print("oracle poses per stream", poses, "brute force (stream 0)", [bool(r["used_bruteforce"]) for r in ro[0]])
    assert any(r["used_bruteforce"] for r in ro[0][1:]) and not all(r["updated"] for r in ro[0])
    assert poses[0] >= 9 and poses[1] >= 9 and poses[2] == N_FRAMES, poses
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
            assert np.array_equal(d_mono[j][5].cpu().numpy(), wit.to_mono8(raw[j][5], encoding)), j
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
        assert [bool(x) for x in info[0, :, 7]] == [bool(r["used_bruteforce"]) for r in ro[0]]
        assert [bool(s == 0) for s in rec["status"][0]] == [bool(r["updated"]) for r in ro[0]]
    finally:
        for t in made:
            t.close()
        h.close()


@pytest.mark.gpu
def test_wide_entry_on_a_bayer_frame_of_70_spots(hip, orc):
    """One mpe_track_step_batch_wide call with a device Bayer frame whose (whole-image) ROI holds 70 spots — by the
    oracle's find_leds over the witness-decoded frame — equals the same call over the converted mono8 frame."""
    import torch
    from test_wide_frames import grid_frame, GRID_ROWS, GRID_COLS
    K, D = synth.camera_for(GRID_ROWS, GRID_COLS)
    gray = grid_frame(np.random.default_rng(70), 70)
    raw = wit.mosaic(gray, "bayer_bggr8", 71)
    und, _ = orc.find_leds(wit.to_mono8(raw, "bayer_bggr8"), orc.make_params(), K, D)
    assert len(und) == 70, len(und)
    roi, setup = (0, 0, GRID_COLS, GRID_ROWS), [(synth.M4, K, D, mpe.demo_params())]
    d_raw = torch.from_numpy(raw).cuda()
    d_mono = hip.convert_to_mono8(d_raw[None], "bayer_bggr8")[0]
    before = hip.get_option("wide_track_submits")
    a = hip.track_step_batch_wide([d_raw], [roi], [None], setup, None, encoding="bayer_bggr8")
    b = hip.track_step_batch_wide([d_mono], [roi], [None], setup, None)
    assert hip.get_option("wide_track_submits") == before + 2
    assert a[0]["n"][0] == 70 and a[0]["status"][0] == 0, (a[0]["n"], a[0]["status"])
    assert np.array_equal(a[0]["undist_xy"][0][:140].reshape(-1, 2), und)
    for k, what in enumerate(("detections", "correspondences", "records")):
        assert a[k].tobytes() == b[k].tobytes(), what


@pytest.mark.gpu
def test_sensor_submit_refusals_leave_the_handle_usable():
    """On a device: encodings 6, 15, 22 and -1 are MPE_ERR_UNSUPPORTED (the encoded entry, mpe_convert_to_mono8, the
    formats entry, the wide entry and the tracker entry), a YUV stride of 2 * cols - 1 and a Bayer stride of cols - 1 are
    MPE_ERR_ARG, nothing is submitted by any of them and the handle gives the reference records afterwards; a Bayer
    image that ends one byte before its allocation's end (and one that ends with it) is accepted."""
    import torch
    lib = mpe.load_library()
    q = synth.make_sequence("C2", 1, seed=990)
    rows, cols = int(q["rows"]), int(q["cols"])
    raw_b = wit.mosaic(q["frames"][0], "bayer_rggb8", 5)
    raw_y = wit.mosaic(q["frames"][0], "yuv422", 6)
    n_b = rows * cols
    d_buf = torch.full((n_b + 1,), GUARD, dtype=torch.uint8).cuda()      # the image ends one byte before the allocation's end
    d_buf[:n_b] = torch.from_numpy(raw_b.reshape(-1)).cuda()
    d_end = torch.full((n_b + 1,), GUARD, dtype=torch.uint8).cuda()      # ... and one that ends with it, 1 byte in
    d_end[1:] = torch.from_numpy(raw_b.reshape(-1)).cuda()
    d_yuv = torch.from_numpy(raw_y).cuda()
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
    RGGB, YUV = CODES["bayer_rggb8"], CODES["yuv422"]

    def items(p):
        it = (mpe.binding.TrackItem * 2)()
        it[0] = mpe.binding.TrackItem(p, 0, 0, cols, rows, None)                            # whole image, detection only
        it[1] = mpe.binding.TrackItem(p, x0, y0, x1 - x0, y1 - y0, pred.ctypes.data)        # tracked around the LEDs
        return it

    def submit(p, stride=cols, enc=RGGB):
        return lib.mpe_track_step_batch_setups_device_encoded_submit(hp, items(p), None, 2, rows, cols, stride, enc, 0, su, 1)

    def collect():
        dets, corr, res = np.zeros(2, mpe.DETECTIONS_DTYPE), np.zeros(2 * 32, np.uint32), np.zeros(2, mpe.RESULT_DTYPE)
        assert lib.mpe_track_step_batch_collect(hp, ctypes.c_void_p(dets.ctypes.data), ctypes.c_void_p(corr.ctypes.data),
                                                ctypes.c_void_p(res.ctypes.data)) == 0
        assert res["status"][1] == 0 and dets["n"][0] == 5
        return dets.tobytes() + corr.tobytes() + res.tobytes()

    d = d_buf.data_ptr()
    try:
        assert submit(d) == 0                       # (ends one byte before the allocation's end)
        ref = collect()
        assert submit(d_end.data_ptr() + 1) == 0    # (ends with the allocation)
        assert collect() == ref
        # ... which are the records of the mono8 device entry over the converted frame
        mono = torch.from_numpy(wit.to_mono8(raw_b, "bayer_rggb8")).cuda()
        torch.cuda.synchronize()
        assert lib.mpe_track_step_batch_setups_device_submit(hp, items(mono.data_ptr()), None, 2, rows, cols, cols, su, 1) == 0
        assert collect() == ref
        n0 = h.get_option("track_batch_submits")
        cases = [(dict(p=d, enc=6), MPE_ERR_UNSUPPORTED, "encoding not supported"),
                 (dict(p=d, enc=15), MPE_ERR_UNSUPPORTED, "encoding not supported"),
                 (dict(p=d, enc=22), MPE_ERR_UNSUPPORTED, "encoding not supported"),
                 (dict(p=d, enc=-1), MPE_ERR_UNSUPPORTED, "encoding not supported"),
                 (dict(p=d_yuv.data_ptr(), enc=YUV, stride=2 * cols - 1), MPE_ERR_ARG, "bad argument"),
                 (dict(p=d, stride=cols - 1), MPE_ERR_ARG, "bad argument")]
        for kw, code, text in cases:
            assert submit(**kw) == code, (kw, code)
            assert text in lib.mpe_last_error(hp).decode(), lib.mpe_last_error(hp).decode()
            assert h.get_option("track_batch_submits") == n0, kw
            assert submit(d) == 0 and collect() == ref, kw
            n0 += 1
        # a YUV frame with its full stride is accepted
        assert submit(d_yuv.data_ptr(), 2 * cols, YUV) == 0
        collect()
        # the other entries answer the same codes
        out = torch.empty(n_b, dtype=torch.uint8).cuda()
        fmts2 = lambda e: (mpe.ImageFormat * 2)(mpe.ImageFormat(rows, cols, cols, e, 0), mpe.ImageFormat(rows, cols, cols, 0, 0))
        idx = (ctypes.c_int * 2)(0, 1)
        for e in (6, 15, 22, -1):
            assert lib.mpe_convert_to_mono8(hp, ctypes.c_void_p(d), 1, e, 0, 1, rows, cols, cols, n_b,
                                            ctypes.c_void_p(out.data_ptr()), 1) == MPE_ERR_UNSUPPORTED, e
            assert lib.mpe_track_step_batch_formats_submit(hp, items(d), None, idx, 2, fmts2(e), 2, 1, su, 1) == MPE_ERR_UNSUPPORTED, e
        # host frames beside a sensor encoding: MPE_ERR_UNSUPPORTED (what the codes answered before); beside bgr8: MPE_ERR_ARG
        host = np.zeros((rows, cols * 3), np.uint8)
        assert lib.mpe_track_step_batch_formats_submit(hp, items(host.ctypes.data), None, idx, 2, fmts2(RGGB), 2, 0, su, 1) == MPE_ERR_UNSUPPORTED
        assert lib.mpe_track_step_batch_formats_submit(hp, items(host.ctypes.data), None, idx, 2, fmts2(YUV), 2, 0, su, 1) == MPE_ERR_UNSUPPORTED
        assert lib.mpe_track_step_batch_formats_submit(hp, items(host.ctypes.data), None, idx, 2, fmts2(1), 2, 0, su, 1) == MPE_ERR_ARG
        assert lib.mpe_convert_to_mono8(hp, ctypes.c_void_p(d_yuv.data_ptr()), 1, YUV, 0, 1, rows, cols, 2 * cols - 1, 2 * n_b,
                                        ctypes.c_void_p(out.data_ptr()), 1) == MPE_ERR_ARG
        t = mpe.Tracker(h, markers, K, D, P)
        times = np.zeros(1)
        tp = times.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        call = lib.mpe_tracker_estimate_batch_device_encoded
        rc22 = call((ctypes.c_void_p * 1)(t._t), 1, (ctypes.c_void_p * 1)(d), rows, cols, cols, 22, 0, tp, None, None, None)
        rc_s = call((ctypes.c_void_p * 1)(t._t), 1, (ctypes.c_void_p * 1)(d_yuv.data_ptr()), rows, cols, 2 * cols - 1, YUV, 0, tp,
                    None, None, None)
        t.close()
        assert rc22 == MPE_ERR_UNSUPPORTED and rc_s == MPE_ERR_ARG
        assert h.get_option("track_batch_submits") == n0 + 1
        assert submit(d) == 0 and collect() == ref
    finally:
        lib.mpe_track_step_batch_cancel(hp)
        h.close()
