"""The one image-format check behind every tracked entry (csrc/mpe_pixel.h: check_format_shape, check_image_format,
image_extent, same_image_format).

CPU tier: the table of refusals, the extents and the equality of formats, as a stand-alone host program under
AddressSanitizer + UBSan (tests/host/image_format_host.cpp) — these functions need no handle.

GPU tier: the uniform device entries of the trackers refuse an image without rows (and, for mono8, without columns or
with a stride below cols) BEFORE a tracker's state is touched; the submission refused the same calls with the same
code and text, but only after the frame had begun (predicted time and ROI already advanced)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from rpg_monocular_pose_estimator_amd import synth
import rpg_monocular_pose_estimator_amd as mpe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")
MPE_ERR_ARG = -1
ROWS = COLS = 64


def test_image_format_checks_on_the_host_under_sanitizers(tmp_path):
    """Every MPE_ENC_* code and four codes outside them, for host and for device frames: code and text; rows = 0,
    cols = 0, stride = cols * bpp - 1 refused and stride = cols * bpp accepted; which refusal answers when two rules
    fail; image_extent per bytes-per-pixel value, for one row and beyond 2^32; same_image_format reads the byte order
    for mono16 alone."""
    exe = str(tmp_path / "image_format_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "host", "image_format_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "image_format_host ok: 12 encodings + 4 unknown codes" in r.stdout, r.stdout


# ---- GPU tier -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _scene():
    """A 64 x 64 frame with the five LEDs of M5, at least 11 pixels apart and 9 from the border"""
    K, D = np.array([[300.0, 0, 32], [0, 300.0, 32], [0, 0, 1]]), np.zeros(5)
    rng = np.random.default_rng(7)
    _, spots = synth.sample_scene(rng, synth.M5, K, D, ROWS, COLS, 0, min_sep=11.0, margin=9.0)
    return synth.render_frame(rng, spots, ROWS, COLS), K, D


def _state(lib, t):
    st = C.create_string_buffer(1024)
    assert lib.mpe_tracker_get_state(t._t, st) == 0
    return st.raw


# entry, its encoding arguments, bytes per pixel; the arguments that are refused earlier than before
ENTRIES = [("mpe_tracker_estimate_batch_device", (), 1), ("mpe_tracker_estimate_batch_device_encoded", (0, 0), 1),
           ("mpe_tracker_estimate_batch_device_encoded", (1, 0), 3),
           ("mpe_tracker_run_sequences_batch_device_threads", (), 1),
           ("mpe_tracker_run_sequences_batch_device_encoded_threads", (0, 0), 1),
           ("mpe_tracker_run_sequences_batch_device_encoded_threads", (1, 0), 3)]
MOVED = [(e, bad) for e in range(len(ENTRIES)) for bad in ("rows", "cols", "stride") if ENTRIES[e][2] == 1 or bad == "rows"]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,bad", MOVED, ids=["%s%s-%s" % (ENTRIES[e][0][12:], ENTRIES[e][1], b) for e, b in MOVED])
def test_device_entries_refuse_a_bad_size_before_the_tracker_is_touched(entry, bad):
    """One tracker, one 64 x 64 device frame.  The refused call (MPE_ERR_ARG, "bad argument") leaves
    mpe_tracker_get_state as it was, and the next valid frame is answered as a fresh tracker answers it."""
    import torch
    name, enc, bpp = ENTRIES[entry]
    frame, K, D = _scene()
    d_mono = torch.from_numpy(frame).cuda()
    d_src = d_mono if bpp == 1 else torch.from_numpy(np.repeat(frame[:, :, None], 3, axis=2).copy()).cuda()
    torch.cuda.synchronize()
    lib = mpe.load_library()
    h = mpe.Handle(0)
    made = []
    try:
        t, fresh = [mpe.Tracker(h, synth.M5, K, D, mpe.demo_params()) for _ in range(2)]
        made += [t, fresh]
        before = _state(lib, t)
        rows, cols, stride = ROWS, COLS, COLS * bpp
        if bad == "rows":
            rows = 0
        elif bad == "cols":
            cols = 0
        else:
            stride = COLS * bpp - 1
        ts, ptrs = (C.c_void_p * 1)(t._t), (C.c_void_p * 1)(d_src.data_ptr())
        times = np.array([5.0])
        tp = times.ctypes.data_as(C.POINTER(C.c_double))
        if "run_sequences" in name:
            rc = getattr(lib, name)(ts, 1, ptrs, 1, rows, cols, stride, ROWS * COLS * bpp, *enc, tp, None, None, 1)
        else:
            rc = getattr(lib, name)(ts, 1, ptrs, rows, cols, stride, *enc, tp, None, None, None)
        assert rc == MPE_ERR_ARG and "bad argument" in lib.mpe_last_error(h._h).decode(), (rc, lib.mpe_last_error(h._h))
        assert _state(lib, t) == before
        got = mpe.tracker_estimate_batch_device([t], [d_mono], [5.0])
        ref = mpe.tracker_estimate_batch_device([fresh], [d_mono], [5.0])
        assert got[0].tobytes() == ref[0].tobytes() and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
        assert ref[1][0, 5] == 5, ref[1]                       # (the five LEDs were found)
        assert _state(lib, t) == _state(lib, fresh)
    finally:
        for x in made:
            x.close()
        h.close()
