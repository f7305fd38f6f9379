"""ctypes binding of libmpe_hip.so (include/mpe.h)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_LIB = os.environ.get("MPE_LIB") or os.path.join(_HERE, "libmpe_hip.so")  # MPE_LIB: kernel-variant experiments
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "mpe.h")

MAX_MARKERS = 16
MAX_DETECTIONS = int(os.environ.get("MPE_MAX_DET", "64"))  # (MPE_MAX_DET: A/B runs against a library built with another capacity)
WIDE_DETECTIONS = 256  # MPE_WIDE_DETECTIONS: detections of one set in the *_wide entries


class MpeError(RuntimeError):
    pass


class MpeParams(C.Structure):
    _fields_ = [
        ("threshold_value", C.c_int),
        ("gaussian_sigma", C.c_double),
        ("min_blob_area", C.c_double),
        ("max_blob_area", C.c_double),
        ("max_width_height_distortion", C.c_double),
        ("max_circular_distortion", C.c_double),
        ("back_projection_pixel_tolerance", C.c_double),
        ("nearest_neighbour_pixel_tolerance", C.c_double),
        ("certainty_threshold", C.c_double),
        ("valid_correspondence_threshold", C.c_double),
        ("roi_border_thickness", C.c_uint),
        ("histogram_threshold", C.c_uint),
    ]


class MpeResult(C.Structure):
    _fields_ = [("T", C.c_double * 16), ("cov", C.c_double * 36), ("status", C.c_int), ("n_det", C.c_int),
                ("n_corr", C.c_int), ("gn_iterations", C.c_int)]


class MpeDetections(C.Structure):
    _fields_ = [("n", C.c_int), ("status", C.c_int), ("undist_xy", C.c_double * (2 * MAX_DETECTIONS)),
                ("dist_xy", C.c_float * (2 * MAX_DETECTIONS))]


class MpeDetectionsWide(C.Structure):  # mpe_detections_wide
    _fields_ = [("n", C.c_int), ("status", C.c_int), ("undist_xy", C.c_double * (2 * WIDE_DETECTIONS)),
                ("dist_xy", C.c_float * (2 * WIDE_DETECTIONS))]


RIG_MAX_CAMERAS = 16  # MPE_RIG_MAX_CAMERAS


class MpeRigCamera(C.Structure):  # mpe_rig_camera
    _fields_ = [("K", C.c_double * 9), ("T_cam_rig", C.c_double * 16)]


class MpeRigTrackOptions(C.Structure):  # mpe_rig_track_options
    _fields_ = [("max_rounds", C.c_int), ("min_rows", C.c_int), ("min_markers", C.c_int)]


class MpeRigTrackInfo(C.Structure):  # mpe_rig_track_info
    _fields_ = [("rounds", C.c_int), ("rows", C.c_int), ("distinct_markers", C.c_int), ("reason", C.c_int),
                ("max_residual", C.c_double), ("rms", C.c_double)]


RIG_TRACK_INFO_DTYPE = np.dtype([("rounds", "i4"), ("rows", "i4"), ("distinct_markers", "i4"), ("reason", "i4"),
                                 ("max_residual", "f8"), ("rms", "f8")])
assert RIG_TRACK_INFO_DTYPE.itemsize == C.sizeof(MpeRigTrackInfo)


class MpeRigInitOptions(C.Structure):  # mpe_rig_init_options
    _fields_ = [("max_rounds", C.c_int), ("min_rows", C.c_int), ("min_markers", C.c_int), ("min_margin", C.c_int)]


class MpeRigInitInfo(C.Structure):  # mpe_rig_init_info
    _fields_ = [("reason", C.c_int), ("camera", C.c_int), ("detection", C.c_int * 3), ("marker", C.c_int * 3),
                ("root", C.c_int), ("best_rows", C.c_int), ("runner_rows", C.c_int), ("best_markers", C.c_int),
                ("n_items", C.c_int64), ("best_sum2", C.c_double), ("T_hyp", C.c_double * 16), ("track", MpeRigTrackInfo)]


RIG_INIT_INFO_DTYPE = np.dtype([("reason", "i4"), ("camera", "i4"), ("detection", "i4", (3,)), ("marker", "i4", (3,)),
                                ("root", "i4"), ("best_rows", "i4"), ("runner_rows", "i4"), ("best_markers", "i4"),
                                ("n_items", "i8"), ("best_sum2", "f8"), ("T_hyp", "f8", (16,)),
                                ("track", RIG_TRACK_INFO_DTYPE)])
assert RIG_INIT_INFO_DTYPE.itemsize == C.sizeof(MpeRigInitInfo) == 224


class MpeRigBody(C.Structure):  # mpe_rig_body
    _fields_ = [("markers_xyz", C.POINTER(C.c_double)), ("n_markers", C.c_int), ("options", C.POINTER(MpeRigInitOptions))]


MAX_BODIES = 16  # MPE_MAX_BODIES


class MpeRigCalibrationOptions(C.Structure):  # mpe_rig_calibration_options
    _fields_ = [("reference_camera", C.c_int), ("max_iterations", C.c_int), ("step_tolerance", C.c_double)]


class MpeRigCalibrationReport(C.Structure):  # mpe_rig_calibration_report
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("views_used", C.c_int), ("rows_used", C.c_int),
                ("rms_before", C.c_double), ("rms_after", C.c_double), ("last_step", C.c_double),
                ("camera_state", C.c_int * RIG_MAX_CAMERAS), ("camera_rows", C.c_int * RIG_MAX_CAMERAS)]


class MpeBodyCalibrationOptions(C.Structure):  # mpe_body_calibration_options
    _fields_ = [("scale", C.c_int), ("max_iterations", C.c_int), ("step_tolerance", C.c_double)]


class MpeBodyCalibrationReport(C.Structure):  # mpe_body_calibration_report
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("views_used", C.c_int), ("rows_used", C.c_int),
                ("markers_free", C.c_int), ("scale_held", C.c_int),
                ("rms_before", C.c_double), ("rms_after", C.c_double), ("last_step", C.c_double),
                ("marker_state", C.c_int * MAX_MARKERS), ("marker_rows", C.c_int * MAX_MARKERS)]


RESULT_DTYPE = np.dtype([("T", "f8", (16,)), ("cov", "f8", (36,)), ("status", "i4"), ("n_det", "i4"),
                         ("n_corr", "i4"), ("gn_iterations", "i4")])
DETECTIONS_DTYPE = np.dtype([("n", "i4"), ("status", "i4"), ("undist_xy", "f8", (2 * MAX_DETECTIONS,)),
                             ("dist_xy", "f4", (2 * MAX_DETECTIONS,))])
assert RESULT_DTYPE.itemsize == C.sizeof(MpeResult)
DETECTIONS_WIDE_DTYPE = np.dtype([("n", "i4"), ("status", "i4"), ("undist_xy", "f8", (2 * WIDE_DETECTIONS,)),
                                  ("dist_xy", "f4", (2 * WIDE_DETECTIONS,))])
assert DETECTIONS_DTYPE.itemsize == C.sizeof(MpeDetections)
assert DETECTIONS_WIDE_DTYPE.itemsize == C.sizeof(MpeDetectionsWide)


def library_path():
    return _LIB


def build_library(force=False):
    """Compile the HIP library for gfx950 with hipcc (csrc/Makefile).  Works without a GPU."""
    cmd = ["make", "-s", "-j4", "-C", _CSRC] + (["-B"] if force else [])
    subprocess.check_call(cmd)
    if not os.path.exists(_LIB):
        raise MpeError("build did not produce %s" % _LIB)
    return _LIB


# the kernel sources, in the order in which they read as one text (the former single file mpe_kernels.hip)
DEVICE_SOURCES = ("mpe_kernels_common.h", "mpe_k1.hip", "mpe_k2_head.h", "mpe_k2.hip", "mpe_k3.hip")


def device_source():
    """The kernel sources as ONE text, file prologues / epilogues (`//@file-prologue` .. `-end`, `//@file-epilogue` ..
    `-end`) dropped: what the CPU tier cuts its host builds of the device code from."""
    out = []
    for name in DEVICE_SOURCES:
        with open(os.path.join(_CSRC, name)) as fh:
            txt = fh.read()
        txt = re.sub(r"//@file-prologue\n.*?//@file-prologue-end\n", "", txt, flags=re.S)
        txt = re.sub(r"//@file-epilogue\n.*?//@file-epilogue-end\n", "", txt, flags=re.S)
        # the blob extraction's device functions live in a header both mpe_k1.hip and mpe_k3.hip include (round 6):
        # its marked body stands where mpe_k1.hip includes it, the second include (mpe_k3.hip) is dropped
        if "//@include-k1b-dev" in txt:
            with open(os.path.join(_CSRC, "mpe_k1b_dev.h")) as fh:
                hdr = fh.read()
            body = hdr[hdr.index("//@k1b-dev-begin\n") + len("//@k1b-dev-begin\n"):hdr.index("//@k1b-dev-end\n")]
            txt = re.sub(r"//@include-k1b-dev.*?//@include-k1b-dev-end\n", lambda m: body, txt, count=1, flags=re.S)
        out.append(txt)
    return "".join(out)


def source_fingerprint():
    """sha256 (16 hex digits) over the kernel / ABI sources of libmpe_hip.so: ties committed profiler passes
    (profiles/round3_pmc.json) to the code a bench run times."""
    import hashlib
    hsh = hashlib.sha256()
    for name in DEVICE_SOURCES + ("mpe_k1b_dev.h", "mpe_ddmath.h", "mpe_ddmath_eval.h", "mpe_p3p.h", "mpe_internal.h", "mpe_host.h", "mpe_schedule.cpp",
                                  "mpe_options.cpp", "mpe_track_abi.cpp", "mpe_abi.cpp", "mpe_track_device.hip",
                                  "mpe_gather.h", "mpe_pixel.h", "mpe_brute_blocks.h", "mpe_wide_peel.h", "mpe_wide.cpp",
                                  "mpe_wide_nn.h", "mpe_rig_gn.h", "mpe_rig_track.h", "mpe_rig_init.h", "mpe_rig.cpp", "mpe_rig_ba.h", "mpe_rig_ba_dev.h",
                                  "mpe_rig_peel.h", "mpe_rig_peel.hip", "mpe_rig_ba_plan.h", "mpe_body_ba.h", "mpe_body_ba_dev.h", "mpe_body_ba_plan.h"):
        with open(os.path.join(_CSRC, name), "rb") as fh:
            hsh.update(fh.read())
    return hsh.hexdigest()[:16]


def exported_symbols():
    """Function names declared in include/mpe.h (used by the symbol-export test)."""
    txt = open(_HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mpe_[a-z0-9_]+)\s*\(", txt)))


_lib = None


def load_library():
    """dlopen libmpe_hip.so.  Raises MpeError when it has not been built — no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise MpeError("%s is missing: run __graft_entry__.build() / make -C %s (there is no CPU fallback)"
                       % (_LIB, _CSRC))
    try:
        import torch  # noqa: F401  (so that one HIP runtime — the one torch loaded — serves both)
    except Exception:
        pass
    lib = C.CDLL(_LIB)
    lib.mpe_version.restype = C.c_char_p
    lib.mpe_last_error.restype = C.c_char_p
    lib.mpe_last_error.argtypes = [C.c_void_p]
    lib.mpe_get_stream.restype = C.c_void_p
    lib.mpe_get_stream.argtypes = [C.c_void_p]
    lib.mpe_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    lib.mpe_destroy.argtypes = [C.c_void_p]
    lib.mpe_destroy.restype = None
    lib.mpe_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.mpe_synchronize.argtypes = [C.c_void_p]
    lib.mpe_set_profiling.argtypes = [C.c_void_p, C.c_int]
    lib.mpe_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    lib.mpe_last_launch_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mpe_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lib.mpe_default_params.argtypes = [C.POINTER(MpeParams)]
    lib.mpe_default_params.restype = None
    dp = C.POINTER(C.c_double)
    lib.mpe_find_leds.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.POINTER(MpeParams), dp, dp, C.c_int, dp, C.POINTER(C.c_float), C.c_int,
                                  C.POINTER(C.c_int)]
    lib.mpe_solve_bruteforce.argtypes = [C.c_void_p, dp, C.c_int, dp, C.c_int, dp, C.POINTER(MpeParams),
                                         C.POINTER(MpeResult), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.mpe_ddmath_batch.argtypes = [C.c_void_p, C.c_int, dp, dp, C.c_int, dp]
    ip, up = C.POINTER(C.c_int), C.POINTER(C.c_uint32)
    lib.mpe_solve_bruteforce_batch.argtypes = [C.c_void_p, dp, ip, C.c_int, dp, C.c_int, dp, C.POINTER(MpeParams),
                                               C.c_void_p, up, up]
    lib.mpe_solve_bruteforce_batch_setups.argtypes = [C.c_void_p, dp, ip, ip, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                      up, up]
    lib.mpe_estimate_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t,
                                       C.c_int, dp, C.c_int, dp, dp, C.c_int, C.POINTER(MpeParams), C.c_void_p]
    lib.mpe_estimate_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, dp, C.c_int, dp, dp,
                                              C.c_int, C.POINTER(MpeParams), C.c_void_p]
    lib.mpe_estimate_batch_device_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, dp, C.c_int, dp,
                                                     dp, C.c_int, C.POINTER(MpeParams), C.c_void_p, C.c_void_p, C.c_int]
    lib.mpe_estimate_batch_device_collect.argtypes = [C.c_void_p, C.c_void_p]
    lib.mpe_stream_next_ready.argtypes = [C.c_void_p, C.c_void_p]
    lib.mpe_stream_drop_prefetch.argtypes = [C.c_void_p]
    lib.mpe_track_step_batch_collect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mpe_track_step_batch_cancel.argtypes = [C.c_void_p]
    lib.mpe_estimate_batch_multi_device_gather.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, dp,
                                                           C.c_int, dp, dp, C.c_int, C.POINTER(MpeParams), C.c_void_p,
                                                           C.POINTER(C.c_int)]
    lib.mpe_convert_to_mono8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_size_t, C.c_size_t, C.c_void_p, C.c_int]
    lib.mpe_detect_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int,
                                     dp, dp, C.c_int, C.POINTER(MpeParams), C.c_void_p]
    lib.mpe_vote_batch.argtypes = [C.c_void_p, dp, C.POINTER(C.c_int), C.c_int, dp, C.c_int, dp, C.c_double,
                                   C.POINTER(C.c_uint32)]
    lib.mpe_vote_batch_wide.argtypes = lib.mpe_vote_batch.argtypes
    lib.mpe_detect_batch_wide.argtypes = lib.mpe_detect_batch.argtypes
    lib.mpe_estimate_batch_wide.argtypes = lib.mpe_estimate_batch.argtypes
    lib.mpe_solve_bruteforce_batch_wide.argtypes = lib.mpe_solve_bruteforce_batch.argtypes
    lib.mpe_vote_items.argtypes = [C.c_void_p, dp, C.POINTER(C.c_int), C.c_int, dp, C.c_int, dp, C.c_double,
                                   C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint32)]
    lib.mpe_check_and_refine.argtypes = [C.c_void_p, dp, C.c_int, dp, C.c_int, dp, C.POINTER(MpeParams),
                                         C.POINTER(C.c_uint32), C.c_int, C.POINTER(MpeResult)]
    lib.mpe_tracker_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.mpe_tracker_destroy.argtypes = [C.c_void_p]
    lib.mpe_tracker_destroy.restype = None
    lib.mpe_tracker_set_markers.argtypes = [C.c_void_p, dp, C.c_int]
    lib.mpe_tracker_set_camera.argtypes = [C.c_void_p, dp, dp, C.c_int]
    lib.mpe_tracker_set_params.argtypes = [C.c_void_p, C.POINTER(MpeParams)]
    lib.mpe_tracker_reset.argtypes = [C.c_void_p]
    lib.mpe_tracker_estimate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_double,
                                         C.POINTER(MpeResult), C.POINTER(C.c_int)]
    lib.mpe_tracker_run_sequence.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t,
                                             C.c_size_t, dp, C.c_void_p, C.c_void_p]
    lib.mpe_alloc_pinned.restype = C.c_void_p
    lib.mpe_alloc_pinned.argtypes = [C.c_size_t]
    lib.mpe_free_pinned.restype = None
    lib.mpe_free_pinned.argtypes = [C.c_void_p]
    hp = C.POINTER(C.c_void_p)
    lib.mpe_tracker_estimate_batch.argtypes = [hp, C.c_int, hp, C.c_int, C.c_int, C.c_size_t, dp, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
    lib.mpe_tracker_run_sequences_batch.argtypes = [hp, C.c_int, hp, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t,
                                                    dp, C.c_void_p, C.c_void_p]
    lib.mpe_tracker_run_sequences_batch_threads.argtypes = [hp, C.c_int, hp, C.c_int, C.c_int, C.c_int, C.c_size_t,
                                                            C.c_size_t, dp, C.c_void_p, C.c_void_p, C.c_int]
    lib.mpe_tracker_estimate_batch_mixed.argtypes = lib.mpe_tracker_estimate_batch.argtypes
    lib.mpe_tracker_run_sequences_batch_mixed_threads.argtypes = lib.mpe_tracker_run_sequences_batch_threads.argtypes
    lib.mpe_tracker_estimate_batch_device.argtypes = lib.mpe_tracker_estimate_batch.argtypes
    lib.mpe_tracker_run_sequences_batch_device_threads.argtypes = lib.mpe_tracker_run_sequences_batch_threads.argtypes
    lib.mpe_track_step_batch_setups_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                                       C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mpe_track_step_batch_setups_device_submit.argtypes = lib.mpe_track_step_batch_setups_device.argtypes[:9]
    # ... in the camera's own encoding: (encoding, src_big_endian) behind the stride(s)
    enc = [C.c_int, C.c_int]
    a = lib.mpe_track_step_batch_setups_device.argtypes
    lib.mpe_track_step_batch_setups_device_encoded.argtypes = a[:7] + enc + a[7:]
    lib.mpe_track_step_batch_setups_device_encoded_submit.argtypes = a[:7] + enc + a[7:9]
    # (frames_on_device, encoding, src_big_endian) behind the stride
    a = lib.mpe_track_step_batch_setups_device.argtypes
    lib.mpe_track_step_batch_wide.argtypes = a[:7] + [C.c_int] + enc + a[7:]
    lib.mpe_tracker_set_wide_frames.argtypes = [C.c_void_p, C.c_int]
    a = lib.mpe_tracker_estimate_batch.argtypes
    lib.mpe_tracker_estimate_batch_device_encoded.argtypes = a[:6] + enc + a[6:]
    a = lib.mpe_tracker_run_sequences_batch_threads.argtypes
    lib.mpe_tracker_run_sequences_batch_device_encoded_threads.argtypes = a[:8] + enc + a[8:]
    # ... every item / stream in an image format of its own (mpe_image_format)
    lib.mpe_track_step_batch_formats.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                                 C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
    lib.mpe_track_step_batch_formats_submit.argtypes = lib.mpe_track_step_batch_formats.argtypes[:10]
    lib.mpe_tracker_estimate_batch_formats.argtypes = [hp, C.c_int, hp, C.c_int, C.c_void_p, dp, C.c_void_p, C.c_void_p,
                                                       C.c_void_p]
    lib.mpe_tracker_run_sequences_batch_formats_threads.argtypes = [hp, C.c_int, hp, C.c_int, C.c_int, C.c_void_p,
                                                                    C.POINTER(C.c_size_t), dp, C.c_void_p, C.c_void_p,
                                                                    C.c_int]
    lib.mpe_shard_bounds.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mpe_shard_bounds.restype = None
    lib.mpe_estimate_batch_multi.argtypes = [hp, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t,
                                             dp, C.c_int, dp, dp, C.c_int, C.POINTER(MpeParams), C.c_void_p]
    lib.mpe_estimate_batch_multi_device.argtypes = [hp, C.c_int, hp, C.POINTER(C.c_int), C.c_int, C.c_int, dp, C.c_int,
                                                    dp, dp, C.c_int, C.POINTER(MpeParams), C.c_void_p]
    # the cameras of a rig fused into one body pose
    lib.mpe_rig_optimise_pose_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, ip, ip, dp, dp, C.c_int, dp, C.c_void_p]
    lib.mpe_rig_fuse_trackers.argtypes = [hp, C.c_int, dp, ip, C.c_void_p, ip]
    lib.mpe_rig_seed_trackers.argtypes = [hp, C.c_int, dp, ip, dp, C.c_double, dp, C.c_double]
    # a body tracked with the whole rig (cameras that see fewer than four LEDs count)
    lib.mpe_rig_track_default_options.argtypes = [C.POINTER(MpeRigTrackOptions)]
    lib.mpe_rig_track_default_options.restype = None
    lib.mpe_rig_track_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, dp, C.c_int, ip, dp, dp, dp, C.c_int, dp,
                                        C.POINTER(MpeRigTrackOptions), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mpe_rig_init_default_options.argtypes = [C.POINTER(MpeRigInitOptions)]
    lib.mpe_rig_init_default_options.restype = None
    lib.mpe_rig_init_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, dp, C.c_int, ip, dp, dp, dp, C.c_int,
                                       C.POINTER(MpeRigInitOptions), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mpe_rig_init_trackers.argtypes = [hp, C.c_int, dp, C.POINTER(MpeRigInitOptions), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mpe_rig_track_trackers.argtypes = [hp, C.c_int, dp, dp, C.POINTER(MpeRigTrackOptions), C.c_void_p, C.c_void_p,
                                           C.c_void_p]
    # several bodies in one frame: rounds of the rig initialiser
    lib.mpe_rig_init_bodies_default_options.argtypes = [C.POINTER(MpeRigInitOptions), C.c_int, C.c_int]
    lib.mpe_rig_init_bodies_default_options.restype = None
    lib.mpe_rig_init_bodies_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(MpeRigBody), C.c_int, ip, dp,
                                              C.c_void_p, C.c_void_p, dp, dp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]
    lib.mpe_rig_init_bodies_trackers.argtypes = [hp, C.c_int, C.c_int, dp, ip, ip, C.c_double, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]
    # the extrinsics of a rig calibrated from the body it tracks
    lib.mpe_rig_calibration_default_options.argtypes = [C.POINTER(MpeRigCalibrationOptions)]
    lib.mpe_rig_calibration_default_options.restype = None
    lib.mpe_rig_calibrate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, ip, ip, dp, dp, C.c_int, dp,
                                      C.POINTER(MpeRigCalibrationOptions), dp, dp, dp, ip, C.POINTER(MpeRigCalibrationReport)]
    lib.mpe_rig_calibration_start.argtypes = [dp, ip, C.c_int, C.c_int, C.c_int, dp, dp, ip]
    # the LED positions of a body calibrated from the sequences it was tracked in
    lib.mpe_body_calibration_default_options.argtypes = [C.POINTER(MpeBodyCalibrationOptions)]
    lib.mpe_body_calibration_default_options.restype = None
    lib.mpe_body_calibrate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, dp, C.c_int, ip, ip, ip, dp, C.c_int, dp,
                                       C.POINTER(MpeBodyCalibrationOptions), dp, dp, dp, ip, C.POINTER(MpeBodyCalibrationReport)]
    lib.mpe_tracker_get_correspondences.argtypes = [C.c_void_p, up, C.c_int]
    lib.mpe_tracker_get_image_points.argtypes = [C.c_void_p, dp, C.c_int]
    _lib = lib
    return lib


def _estimate_batch(name, trackers, ptrs, rows, cols, stride, times, enc=()):
    """One lock-step time step through entry `name`: ptrs = the trackers' images (host or device addresses) of one
    shape and row stride; enc: (encoding, big_endian) for an *_encoded entry.
    -> (records (N), info (N,8), updated (N) bool)."""
    lib = load_library()
    n = len(trackers)
    ts = (C.c_void_p * n)(*[t._t for t in trackers])
    times = _f64(times).reshape(-1)
    rec = np.zeros(n, RESULT_DTYPE)
    info = np.zeros((n, 8), np.int32)
    upd = np.zeros(n, np.int32)
    rc = getattr(lib, name)(ts, n, ptrs, rows, cols, stride, *enc, _dp(times), rec.ctypes.data, info.ctypes.data,
                            upd.ctypes.data)
    if rc < 0:
        raise MpeError("%s failed (%d): %s" % (name, rc, lib.mpe_last_error(trackers[0]._handle._h).decode()))
    return rec, info, upd.astype(bool)


def _run_sequences_batch(name, trackers, ptrs, n, rows, cols, stride, fstride, times, threads, enc=()):
    """The lock-step loop in C through entry `name`: ptrs = the trackers' sequences (host or device addresses) of n
    frames each, one shape, row stride and frame stride; enc: (encoding, big_endian) for an *_encoded entry.
    -> (records (N,n), info (N,n,8))."""
    lib = load_library()
    N = len(trackers)
    ts = (C.c_void_p * N)(*[t._t for t in trackers])
    times = _f64(times).reshape(-1)
    rec = np.zeros((N, n), RESULT_DTYPE)
    info = np.zeros((N, n, 8), np.int32)
    rc = getattr(lib, name)(ts, N, ptrs, n, rows, cols, stride, fstride, *enc, _dp(times), rec.ctypes.data,
                            info.ctypes.data, int(threads))
    if rc < 0:
        raise MpeError("%s failed (%d): %s" % (name, rc, lib.mpe_last_error(trackers[0]._handle._h).decode()))
    return rec, info


def tracker_estimate_batch(trackers, imgs, times, mixed=False):
    """mpe_tracker_estimate_batch: frame k of N trackers (same handle / camera / markers / parameters) in lock step,
    one device submission per step in steady state.  imgs: list of (rows, cols) uint8 arrays; times: N floats.
    mixed: mpe_tracker_estimate_batch_mixed (the trackers may differ in camera, markers and parameters).
    -> (records [RESULT_DTYPE] (N), info (N,8) int32, updated (N) bool)."""
    imgs = [np.ascontiguousarray(im, np.uint8) for im in imgs]
    rows, cols = imgs[0].shape
    stride = imgs[0].strides[0]
    assert all(im.shape == (rows, cols) and im.strides[0] == stride for im in imgs)
    ptrs = (C.c_void_p * len(trackers))(*[im.ctypes.data for im in imgs])
    return _estimate_batch("mpe_tracker_estimate_batch_mixed" if mixed else "mpe_tracker_estimate_batch", trackers, ptrs,
                           rows, cols, stride, times)


def tracker_estimate_batch_mixed(trackers, imgs, times):
    """mpe_tracker_estimate_batch_mixed: as tracker_estimate_batch for distinct trackers on ONE handle that may differ
    in camera (K, D), marker set and parameters — e.g. the cameras of a multi-camera rig."""
    return tracker_estimate_batch(trackers, imgs, times, mixed=True)


def tracker_run_sequences_batch(trackers, frames, times, threads=1, mixed=False):
    """mpe_tracker_run_sequences_batch[_threads]: the lock-step loop in C.  frames: list of (n,rows,cols) uint8 arrays
    (one sequence per tracker), times: n floats; threads > 1: the handle groups on that many host threads.
    mixed: mpe_tracker_run_sequences_batch_mixed_threads (groups by handle alone, each may mix set-ups).
    -> (records (N,n), info (N,n,8))."""
    frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
    n, rows, cols = frames[0].shape
    assert all(f.shape == (n, rows, cols) for f in frames)
    ptrs = (C.c_void_p * len(trackers))(*[f.ctypes.data for f in frames])
    return _run_sequences_batch("mpe_tracker_run_sequences_batch_mixed_threads" if mixed
                                else "mpe_tracker_run_sequences_batch_threads", trackers, ptrs, n, rows, cols,
                                frames[0].strides[1], frames[0].strides[0], times, threads)


def tracker_run_sequences_batch_mixed(trackers, frames, times, threads=1):
    """mpe_tracker_run_sequences_batch_mixed_threads: as tracker_run_sequences_batch, each handle's trackers one
    lock-step group that may mix cameras, marker sets and parameters."""
    return tracker_run_sequences_batch(trackers, frames, times, threads, mixed=True)


def _device_images(imgs, lead, encoding="mono8"):
    """The streams' images in device memory: a list of torch CUDA tensors, one per stream, or one tensor with a leading
    stream dimension; `lead` dimensions in front of the image.  mono8 and the Bayer patterns: (rows, cols) uint8.  Any
    other encoding (ENCODINGS): (rows, cols, bytes per pixel) uint8 with the bytes of a pixel contiguous (YUV 4:2:2: 2),
    or, mono16, (rows, cols) uint16 / int16.  All on one device, pixels contiguous within a row, the same strides; row stride and storage offset
    are free.  Work queued on torch's current stream of that device is waited for (the frames must be final when they
    are submitted).  -> (the tensors — keep them alive across the call —, device pointers, the lead + (rows, cols)
    shape, their strides in BYTES)."""
    import torch
    if encoding not in ENCODINGS:
        raise MpeError("encoding %r: one of %s" % (encoding, ", ".join(sorted(ENCODINGS))))
    bpp = ENCODING_BPP[encoding]
    ts = list(imgs.unbind(0)) if _is_torch(imgs) else list(imgs)
    t0 = ts[0]
    for t in ts:
        ok = _is_torch(t) and t.is_cuda
        if ok and bpp == 1:
            ok = t.dtype == torch.uint8 and t.dim() == lead + 2 and t.stride(-1) == 1
        elif ok and t.dtype == torch.uint8:    # the bytes of a pixel as a last dimension
            ok = t.dim() == lead + 3 and t.shape[-1] == bpp and t.stride(-1) == 1 and t.stride(-2) == bpp
        elif ok:
            ok = encoding == "mono16" and t.dtype in (torch.uint16, torch.int16) and t.dim() == lead + 2 and t.stride(-1) == 1
        if not ok:
            raise MpeError("device frames: torch CUDA tensors with contiguous rows are needed — (rows, cols) uint8 for mono8 / Bayer, "
                           "(rows, cols, bytes per pixel) uint8 or, mono16, (rows, cols) uint16 / int16 for the other "
                           "encodings (host frames: the host entries)")
        if t.shape != t0.shape or t.stride() != t0.stride() or t.device != t0.device or t.dtype != t0.dtype:
            raise MpeError("device frames: every stream needs the same shape, strides and device")
    torch.cuda.current_stream(t0.device).synchronize()
    es = t0.element_size()
    return (ts, (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), tuple(t0.shape[:lead + 2]),
            tuple(s * es for s in t0.stride()[:lead + 2]))


def _enc_args(encoding, big_endian):
    return (ENCODINGS[encoding], int(bool(big_endian)))


def tracker_estimate_batch_device(trackers, imgs, times, encoding="mono8", big_endian=False):
    """mpe_tracker_estimate_batch_device: tracker_estimate_batch[_mixed] for frames that are in device memory — imgs: a
    list of (rows, cols) torch uint8 CUDA tensors, one per tracker, or one (N, rows, cols) tensor, on the device of the
    trackers' handle.  The trackers may mix set-ups.  -> (records (N), info (N,8), updated (N) bool), those of the host
    entries over the same frames.
    encoding other than "mono8" (ENCODINGS; big_endian for "mono16"): mpe_tracker_estimate_batch_device_encoded over
    frames in that encoding — (rows, cols, bytes per pixel) uint8 or, mono16, (rows, cols) uint16 / int16 tensors; the
    records are those of the mono8 call over the frames after Handle.convert_to_mono8."""
    keep, ptrs, (rows, cols), (stride, _) = _device_images(imgs, 0, encoding)  # (keep: alive across the call)
    assert len(keep) == len(trackers)
    if encoding == "mono8":
        return _estimate_batch("mpe_tracker_estimate_batch_device", trackers, ptrs, rows, cols, stride, times)
    return _estimate_batch("mpe_tracker_estimate_batch_device_encoded", trackers, ptrs, rows, cols, stride, times,
                           _enc_args(encoding, big_endian))


def tracker_run_sequences_batch_device(trackers, frames, times, threads=1, encoding="mono8", big_endian=False):
    """mpe_tracker_run_sequences_batch_device_threads: tracker_run_sequences_batch[_mixed] over sequences that are in
    device memory — frames: a list of (n, rows, cols) torch uint8 CUDA tensors, one per tracker, or one (N, n, rows, cols)
    tensor.  Each handle's trackers form one lock-step group that may mix set-ups.  -> (records (N,n), info (N,n,8)).
    encoding other than "mono8": mpe_tracker_run_sequences_batch_device_encoded_threads over sequences in that encoding
    ((n, rows, cols, bytes per pixel) uint8 or, mono16, (n, rows, cols) uint16 / int16), as tracker_estimate_batch_device."""
    keep, ptrs, (n, rows, cols), (fstride, stride, _) = _device_images(frames, 1, encoding)  # (keep: alive across the call)
    assert len(keep) == len(trackers)
    if encoding == "mono8":
        return _run_sequences_batch("mpe_tracker_run_sequences_batch_device_threads", trackers, ptrs, n, rows, cols, stride,
                                    fstride, times, threads)
    return _run_sequences_batch("mpe_tracker_run_sequences_batch_device_encoded_threads", trackers, ptrs, n, rows, cols,
                                stride, fstride, times, threads, _enc_args(encoding, big_endian))


class ImageFormat(C.Structure):  # mpe_image_format
    _fields_ = [("rows", C.c_int), ("cols", C.c_int), ("stride_bytes", C.c_size_t), ("encoding", C.c_int),
                ("src_big_endian", C.c_int)]

    def key(self):
        """What makes two formats the same images (the byte order counts for mono16 alone)."""
        return (self.rows, self.cols, self.stride_bytes, self.encoding,
                bool(self.src_big_endian) if self.encoding == ENCODINGS["mono16"] else False)


def _image_format(img, lead, spec):
    """One image (lead 0) or sequence (lead 1: frames in front) of a *_formats entry: a numpy array (host) or a torch
    CUDA tensor (device).  spec: an ImageFormat, taken as it is; or an encoding name / (name, big_endian) / None
    ("mono8"), and the format is read off the array — (rows, cols) uint8 for mono8 / Bayer, (rows, cols, bytes per pixel) uint8
    or, mono16, (rows, cols) uint16 / int16 for the other encodings, pixels contiguous within a row.
    -> (ImageFormat, address, frame stride in bytes (lead 1, else 0))."""
    dev = _is_torch(img)
    es = img.element_size() if dev else img.itemsize
    strides = [x * es for x in img.stride()] if dev else list(img.strides)
    ptr = img.data_ptr() if dev else img.ctypes.data
    fstride = strides[0] if lead else 0
    if isinstance(spec, ImageFormat):
        return spec, ptr, fstride
    name, big = (spec, False) if spec is None or isinstance(spec, str) else spec
    name = name or "mono8"
    if name not in ENCODINGS:
        raise MpeError("encoding %r: one of %s" % (name, ", ".join(sorted(ENCODINGS))))
    bpp = ENCODING_BPP[name]
    shape, nd = tuple(img.shape), len(img.shape)
    if es == 1 and bpp > 1:
        ok = nd == lead + 3 and shape[-1] == bpp and strides[-1] == 1 and strides[-2] == bpp
    else:
        ok = es == bpp and (es == 1 or name == "mono16") and nd == lead + 2 and strides[-1] == es
    if not ok:
        raise MpeError("%s frames: (rows, cols) uint8 for mono8 / Bayer, (rows, cols, bytes per pixel) uint8 or, mono16, (rows, cols) "
                       "uint16 / int16 for the other encodings, pixels contiguous within a row" % name)
    return (ImageFormat(int(shape[lead]), int(shape[lead + 1]), int(strides[lead]), ENCODINGS[name], int(bool(big))), ptr,
            fstride)


def _stream_formats(imgs, lead, formats):
    """The images (or sequences) of the streams of a *_formats entry, which may differ in shape and strides: all numpy
    (host) or all torch CUDA tensors on one device (work queued on torch's current stream there is waited for).
    -> (frames_on_device, addresses, [ImageFormat], frame strides)."""
    imgs = list(imgs)
    on_device = _is_torch(imgs[0])
    if on_device:
        import torch
        if not all(_is_torch(t) and t.is_cuda and t.device == imgs[0].device for t in imgs):
            raise MpeError("device frames: torch CUDA tensors on one device are needed (no mix with host frames)")
        torch.cuda.current_stream(imgs[0].device).synchronize()
    elif any(_is_torch(t) for t in imgs):
        raise MpeError("host frames: numpy arrays are needed (no mix with device frames)")
    specs = [None] * len(imgs) if formats is None else list(formats)
    assert len(specs) == len(imgs)
    got = [_image_format(im, lead, sp) for im, sp in zip(imgs, specs)]
    return int(on_device), [g[1] for g in got], [g[0] for g in got], [g[2] for g in got]


def tracker_estimate_batch_formats(trackers, imgs, times, formats=None):
    """mpe_tracker_estimate_batch_formats: one lock-step time step of distinct trackers on ONE handle whose cameras may
    differ in image size, row stride and encoding (and in camera, markers and parameters).  imgs: a list of numpy arrays
    (host frames, mono8) or of torch CUDA tensors (device frames), one per tracker, of any shapes.  formats: None (mono8
    formats read off the arrays), or per tracker an encoding name, (name, big_endian) or an ImageFormat.
    -> (records (N), info (N,8), updated (N) bool), those of the existing entries over each format's trackers alone."""
    lib = load_library()
    n = len(trackers)
    on_device, ptrs, fmts, _ = _stream_formats(imgs, 0, formats)
    assert len(ptrs) == n
    ts = (C.c_void_p * n)(*[t._t for t in trackers])
    times = _f64(times).reshape(-1)
    rec, info, upd = np.zeros(n, RESULT_DTYPE), np.zeros((n, 8), np.int32), np.zeros(n, np.int32)
    rc = lib.mpe_tracker_estimate_batch_formats(ts, n, (C.c_void_p * n)(*ptrs), on_device, (ImageFormat * n)(*fmts), _dp(times),
                                                rec.ctypes.data, info.ctypes.data, upd.ctypes.data)
    if rc < 0:
        raise MpeError("mpe_tracker_estimate_batch_formats failed (%d): %s"
                       % (rc, lib.mpe_last_error(trackers[0]._handle._h).decode()))
    return rec, info, upd.astype(bool)


def tracker_run_sequences_batch_formats(trackers, frames, times, threads=1, formats=None):
    """mpe_tracker_run_sequences_batch_formats_threads: the lock-step loop in C over sequences that may differ in image
    size, row stride, frame stride and encoding.  frames: a list of (n, rows, cols[, bytes per pixel]) numpy arrays
    (host, mono8) or torch CUDA tensors (device), one sequence per tracker, the same n; formats as in
    tracker_estimate_batch_formats.  Each handle's trackers form one lock-step group.  -> (records (N,n), info (N,n,8))."""
    lib = load_library()
    N = len(trackers)
    on_device, ptrs, fmts, fstrides = _stream_formats(frames, 1, formats)
    n = int(frames[0].shape[0])
    assert len(ptrs) == N and all(int(f.shape[0]) == n for f in frames)
    ts = (C.c_void_p * N)(*[t._t for t in trackers])
    times = _f64(times).reshape(-1)
    rec, info = np.zeros((N, n), RESULT_DTYPE), np.zeros((N, n, 8), np.int32)
    rc = lib.mpe_tracker_run_sequences_batch_formats_threads(ts, N, (C.c_void_p * N)(*ptrs), n, on_device,
                                                             (ImageFormat * N)(*fmts), (C.c_size_t * N)(*fstrides),
                                                             _dp(times), rec.ctypes.data, info.ctypes.data, int(threads))
    if rc < 0:
        raise MpeError("mpe_tracker_run_sequences_batch_formats_threads failed (%d): %s"
                       % (rc, lib.mpe_last_error(trackers[0]._handle._h).decode()))
    return rec, info


class TrackItem(C.Structure):  # mpe_track_item
    _fields_ = [("img", C.c_void_p), ("roi_x", C.c_int), ("roi_y", C.c_int), ("roi_w", C.c_int), ("roi_h", C.c_int),
                ("predicted_px", C.c_void_p)]


class TrackSetup(C.Structure):  # mpe_track_setup
    _fields_ = [("p", C.c_void_p), ("K", C.c_void_p), ("D", C.c_void_p), ("nD", C.c_int), ("markers_xyz", C.c_void_p),
                ("n_markers", C.c_int)]


class PinnedFrames:
    """(n, rows, cols) uint8 frame buffer in page-locked host memory (mpe_alloc_pinned): `.array` is a numpy view."""

    def __init__(self, n, rows, cols):
        self._lib = load_library()
        self._p = self._lib.mpe_alloc_pinned(n * rows * cols)
        if not self._p:
            raise MpeError("mpe_alloc_pinned(%d) failed" % (n * rows * cols))
        self.array = np.ctypeslib.as_array((C.c_uint8 * (n * rows * cols)).from_address(self._p)).reshape(n, rows, cols)

    def close(self):
        if getattr(self, "_p", None):
            self.array = None
            self._lib.mpe_free_pinned(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_bounds(n_frames, shard, n_shards):
    """mpe_shard_bounds: contiguous chunk [lo, hi) of shard `shard` (host arithmetic, no device)."""
    lo, hi = C.c_int(), C.c_int()
    load_library().mpe_shard_bounds(int(n_frames), int(shard), int(n_shards), C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def estimate_batch_multi(handles, frames, markers, K, D, params):
    """mpe_estimate_batch_multi: one host process, the batch sharded over several handles (= GPUs).
    frames: numpy (n,rows,cols) uint8 on the host, or a LIST of torch uint8 CUDA tensors, one per handle, each
    resident on its handle's device (mpe_estimate_batch_multi_device).  -> numpy records in frame order."""
    lib = load_library()
    markers = _f64(markers).reshape(-1, 3)
    K = _f64(K).reshape(9)
    D = _f64(D).reshape(-1)
    hs = (C.c_void_p * len(handles))(*[h._h for h in handles])
    if isinstance(frames, (list, tuple)):
        assert len(frames) == len(handles)
        rows, cols = frames[0].shape[1:]
        ptrs = (C.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
        counts = (C.c_int * len(frames))(*[f.shape[0] for f in frames])
        out = np.zeros(sum(f.shape[0] for f in frames), RESULT_DTYPE)
        rc = lib.mpe_estimate_batch_multi_device(hs, len(handles), ptrs, counts, rows, cols, _dp(markers), len(markers),
                                                 _dp(K), _dp(D), len(D), C.byref(params), C.c_void_p(out.ctypes.data))
    else:
        frames = np.ascontiguousarray(frames, np.uint8)
        n, rows, cols = frames.shape
        out = np.zeros(n, RESULT_DTYPE)
        rc = lib.mpe_estimate_batch_multi(hs, len(handles), C.c_void_p(frames.ctypes.data), n, rows, cols,
                                          frames.strides[1], frames.strides[0], _dp(markers), len(markers), _dp(K),
                                          _dp(D), len(D), C.byref(params), C.c_void_p(out.ctypes.data))
    if rc != 0:
        msgs = [lib.mpe_last_error(h._h).decode() for h in handles]
        raise MpeError("mpe_estimate_batch_multi failed (%d): %s" % (rc, "; ".join(m for m in msgs if m)))
    return out


def estimate_batch_multi_device_gather(handles, frames, markers, K, D, params):
    """mpe_estimate_batch_multi_device_gather: device-resident shards (a LIST of torch uint8 CUDA tensors, one per
    handle, each on its handle's device) -> ONE torch uint8 tensor of records on handles[0]'s device, gathered GPU to
    GPU (RCCL over xGMI when the handles sit on distinct devices).  -> (records as numpy, used_rccl)."""
    import torch
    lib = load_library()
    markers = _f64(markers).reshape(-1, 3)
    K = _f64(K).reshape(9)
    D = _f64(D).reshape(-1)
    hs = (C.c_void_p * len(handles))(*[h._h for h in handles])
    rows, cols = frames[0].shape[1:]
    ptrs = (C.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
    counts = (C.c_int * len(frames))(*[f.shape[0] for f in frames])
    n = sum(f.shape[0] for f in frames)
    out = torch.zeros(n * RESULT_DTYPE.itemsize, dtype=torch.uint8, device=frames[0].device)
    torch.cuda.synchronize()
    used = C.c_int(0)
    rc = lib.mpe_estimate_batch_multi_device_gather(hs, len(handles), ptrs, counts, rows, cols, _dp(markers), len(markers),
                                                    _dp(K), _dp(D), len(D), C.byref(params), C.c_void_p(out.data_ptr()),
                                                    C.byref(used))
    if rc != 0:
        msgs = [lib.mpe_last_error(h._h).decode() for h in handles]
        raise MpeError("mpe_estimate_batch_multi_device_gather failed (%d): %s" % (rc, "; ".join(m for m in msgs if m)))
    return np.frombuffer(out.cpu().numpy().tobytes(), RESULT_DTYPE), bool(used.value)


def determine_roi(px, rows, cols, border, K, D):
    """LEDDetector::determineROI (host arithmetic inside libmpe_hip.so; needs no device)."""
    lib = load_library()
    px = _f64(px).reshape(-1, 2)
    K = _f64(K).reshape(9)
    D = _f64(D).reshape(-1)
    roi = (C.c_int * 4)()
    rc = lib.mpe_determine_roi(_dp(px), len(px), int(rows), int(cols), int(border), _dp(K), _dp(D), len(D), roi)
    if rc != 0:
        raise MpeError("mpe_determine_roi failed (%d)" % rc)
    return tuple(roi)


def distort_points(xy, K, D):
    """LEDDetector::distortPoints, float32 in / out (host arithmetic)."""
    lib = load_library()
    s = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    d = np.zeros_like(s)
    K = _f64(K).reshape(9)
    D = _f64(D).reshape(-1)
    rc = lib.mpe_distort_points(s.ctypes.data_as(C.POINTER(C.c_float)), d.ctypes.data_as(C.POINTER(C.c_float)), len(s),
                                _dp(K), _dp(D), len(D))
    if rc != 0:
        raise MpeError("mpe_distort_points failed (%d)" % rc)
    return d


def exponential_map(twist):
    T = np.zeros(16)
    load_library().mpe_exponential_map(_dp(_f64(twist).reshape(6)), _dp(T))
    return T.reshape(4, 4)


def logarithm_map(T):
    xi = np.zeros(6)
    load_library().mpe_logarithm_map(_dp(_f64(T).reshape(16)), _dp(xi))
    return xi


def predict_pose(current, previous, t_current, t_previous, t_predict):
    """predictPose (pose_estimator.cpp:232-244), host arithmetic."""
    out = np.zeros(16)
    lib = load_library()
    lib.mpe_predict_pose.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double,
                                     C.POINTER(C.c_double)]
    lib.mpe_predict_pose(_dp(_f64(current).reshape(16)), _dp(_f64(previous).reshape(16)), t_current, t_previous,
                         t_predict, _dp(out))
    return out.reshape(4, 4)


def project_points(T, markers, K):
    markers = _f64(markers).reshape(-1, 3)
    px = np.zeros((len(markers), 2))
    load_library().mpe_project_points(_dp(_f64(T).reshape(16)), _dp(markers), len(markers), _dp(_f64(K).reshape(9)),
                                      _dp(px))
    return px


def find_correspondences(pred_px, det, tol):
    pred = _f64(pred_px).reshape(-1, 2)
    det = _f64(det).reshape(-1, 2)
    corr = np.zeros((len(pred) + 1, 2), np.uint32)
    lib = load_library()
    lib.mpe_find_correspondences.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int, C.c_double,
                                             C.c_void_p]
    n = lib.mpe_find_correspondences(_dp(pred), len(pred), _dp(det), len(det), float(tol), C.c_void_p(corr.ctypes.data))
    if n < 0:
        raise MpeError("mpe_find_correspondences failed (%d)" % n)
    return corr[:n].copy()


ENCODINGS = {"mono8": 0, "bgr8": 1, "rgb8": 2, "bgra8": 3, "rgba8": 4, "mono16": 5,  # MPE_ENC_*
             "bayer_rggb8": 16, "bayer_bggr8": 17, "bayer_gbrg8": 18, "bayer_grbg8": 19, "yuv422": 20, "yuv422_yuy2": 21}
# source bytes per pixel.  Frames are (rows, cols) uint8 for 1 (mono8, Bayer), (rows, cols, bytes per pixel) uint8 for
# the others (YUV 4:2:2: the pixel's two bytes), or, mono16 alone, (rows, cols) uint16 / int16
ENCODING_BPP = {"mono8": 1, "bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4, "mono16": 2, "bayer_rggb8": 1, "bayer_bggr8": 1,
                "bayer_gbrg8": 1, "bayer_grbg8": 1, "yuv422": 2, "yuv422_yuy2": 2}


def demo_params(**kw):
    """Parameter set of launch/demo.launch:12-22 (overridable by keyword)."""
    p = MpeParams()
    load_library().mpe_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class Handle:
    """One GPU + one HIP stream (mpe_handle)."""

    def __init__(self, device=-1):
        self._lib = load_library()
        self._h = C.c_void_p()
        rc = self._lib.mpe_create(C.byref(self._h), int(device))
        if rc != 0:
            self._h = None
            raise MpeError("mpe_create failed (%d): no usable HIP device — there is no CPU fallback" % rc)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mpe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise MpeError("%s failed (%d): %s" % (what, rc, self._lib.mpe_last_error(self._h).decode()))

    # ---- stream / options -------------------------------------------------------------------
    def set_stream(self, stream_ptr):
        self._check(self._lib.mpe_set_stream(self._h, C.c_void_p(stream_ptr or 0)), "mpe_set_stream")

    def synchronize(self):
        self._check(self._lib.mpe_synchronize(self._h), "mpe_synchronize")

    def get_option(self, name):
        v = C.c_int(0)
        self._check(self._lib.mpe_get_option(self._h, name.encode(), C.byref(v)), "mpe_get_option")
        return v.value

    def set_option(self, name, value):
        self._check(self._lib.mpe_set_option(self._h, name.encode(), int(value)), "mpe_set_option")

    def set_profiling(self, on):
        self._check(self._lib.mpe_set_profiling(self._h, 1 if on else 0), "mpe_set_profiling")

    def last_kernel_ms_sub(self, sub_batch):
        ms = (C.c_float * 4)()
        self._check(self._lib.mpe_last_kernel_ms_sub(self._h, int(sub_batch), ms), "mpe_last_kernel_ms_sub")
        return dict(scan=ms[0], blobs=ms[1], vote=ms[2], tail=ms[3])

    def last_kernel_ms(self):
        ms = (C.c_float * 5)()
        self._check(self._lib.mpe_last_kernel_ms(self._h, ms), "mpe_last_kernel_ms")
        nl, fpl = C.c_int(0), C.c_int(0)
        self._check(self._lib.mpe_last_launch_shape(self._h, C.byref(nl), C.byref(fpl)), "mpe_last_launch_shape")
        return dict(scan=ms[0], blobs=ms[1], vote=ms[2], tail=ms[3], total=ms[4], launches=nl.value,
                    frames_per_launch=fpl.value)

    # ---- LEDDetector::findLeds ----------------------------------------------------------------
    def find_leds(self, img, params, K, D, roi=None, cap=MAX_DETECTIONS):
        img = np.ascontiguousarray(img, np.uint8)
        rows, cols = img.shape
        rx, ry, rw, rh = roi if roi is not None else (0, 0, cols, rows)
        K = _f64(K).reshape(9)
        D = _f64(D).reshape(-1)
        und = np.zeros((cap, 2))
        dst = np.zeros((cap, 2), np.float32)
        n = C.c_int(0)
        rc = self._lib.mpe_find_leds(self._h, img.ctypes.data, rows, cols, img.strides[0], rx, ry, rw, rh,
                                     C.byref(params), _dp(K), _dp(D), len(D), _dp(und),
                                     dst.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n))
        self._check(rc, "mpe_find_leds")
        return und[:n.value].copy(), dst[:n.value].copy()

    # ---- setImagePoints + initialise + optimiseAndUpdatePose ---------------------------------
    def solve_bruteforce(self, det, markers, K, params):
        det = _f64(det).reshape(-1, 2)
        markers = _f64(markers).reshape(-1, 3)
        K = _f64(K).reshape(9)
        res = MpeResult()
        hist = np.zeros((max(len(det), 1), len(markers)), np.uint32)
        corr = np.zeros((len(markers), 2), np.uint32)
        rc = self._lib.mpe_solve_bruteforce(self._h, _dp(det), len(det), _dp(markers), len(markers), _dp(K),
                                            C.byref(params), C.byref(res),
                                            hist.ctypes.data_as(C.POINTER(C.c_uint32)),
                                            corr.ctypes.data_as(C.POINTER(C.c_uint32)))
        self._check(rc, "mpe_solve_bruteforce")
        return dict(status=res.status, T=np.array(res.T).reshape(4, 4), cov=np.array(res.cov).reshape(6, 6),
                    n_det=res.n_det, n_corr=res.n_corr, gn_iterations=res.gn_iterations,
                    hist=hist[:len(det)].copy(), corr=corr[:res.n_corr].copy())

    # ---- the same for N detection sets in one call ----------------------------------------------
    @staticmethod
    def _pack_dets(dets):
        n = len(dets)
        buf = np.zeros((n, MAX_DETECTIONS, 2))
        nd = np.zeros(n, np.int32)
        for i, d in enumerate(dets):
            d = _f64(d).reshape(-1, 2)
            nd[i] = len(d)
            buf[i, :len(d)] = d
        return buf, nd

    def solve_bruteforce_batch(self, dets, markers, K, params):
        """mpe_solve_bruteforce_batch: dets a list of (n_i, 2) arrays, one marker set, camera and parameter set.
        -> (records [RESULT_DTYPE] (N), histograms (N, MAX_DETECTIONS, MAX_MARKERS) uint32, correspondences
        (N, MAX_MARKERS, 2) uint32)."""
        markers, K = _f64(markers).reshape(-1, 3), _f64(K).reshape(9)
        buf, nd = self._pack_dets(dets)
        n = len(nd)
        rec = np.zeros(n, RESULT_DTYPE)
        hist = np.zeros((n, MAX_DETECTIONS, MAX_MARKERS), np.uint32)
        corr = np.zeros((n, MAX_MARKERS, 2), np.uint32)
        up = C.POINTER(C.c_uint32)
        rc = self._lib.mpe_solve_bruteforce_batch(self._h, _dp(buf), nd.ctypes.data_as(C.POINTER(C.c_int)), n, _dp(markers),
                                                  len(markers), _dp(K), C.byref(params), C.c_void_p(rec.ctypes.data),
                                                  hist.ctypes.data_as(up), corr.ctypes.data_as(up))
        self._check(rc, "mpe_solve_bruteforce_batch")
        return rec, hist, corr

    # ---- the *_wide entries: detection sets of up to WIDE_DETECTIONS points ---------------------------
    @staticmethod
    def _pack_dets_wide(dets):
        n = len(dets)
        buf = np.zeros((n, WIDE_DETECTIONS, 2))
        nd = np.zeros(n, np.int32)
        for i, d in enumerate(dets):
            d = _f64(d).reshape(-1, 2)
            nd[i] = len(d)
            buf[i, :min(len(d), WIDE_DETECTIONS)] = d[:WIDE_DETECTIONS]  # (a longer set: the library refuses its count)
        return buf, nd

    @staticmethod
    def _frame_args(frames):
        if _is_torch(frames):
            assert frames.is_cuda and frames.is_contiguous()
            n, rows, cols = frames.shape
            return frames, n, rows, cols, frames.data_ptr(), 1, cols, rows * cols
        frames = np.ascontiguousarray(frames, np.uint8)
        n, rows, cols = frames.shape
        return frames, n, rows, cols, frames.ctypes.data, 0, frames.strides[1], frames.strides[0]

    def detect_batch_wide(self, frames, K, D, params):
        """mpe_detect_batch_wide: frames as for detect_batch.  -> records [DETECTIONS_WIDE_DTYPE] (n)."""
        K, D = _f64(K).reshape(9), _f64(D).reshape(-1)
        frames, n, rows, cols, ptr, on_dev, stride, fstride = self._frame_args(frames)
        out = np.zeros(n, DETECTIONS_WIDE_DTYPE)
        rc = self._lib.mpe_detect_batch_wide(self._h, C.c_void_p(ptr), n, rows, cols, stride, fstride, on_dev, _dp(K),
                                             _dp(D), len(D), C.byref(params), C.c_void_p(out.ctypes.data))
        self._check(rc, "mpe_detect_batch_wide")
        return out

    def estimate_batch_wide(self, frames, markers, K, D, params):
        """mpe_estimate_batch_wide: estimate_batch, with the frames of 65 .. WIDE_DETECTIONS blobs solved by the wide path."""
        markers, K, D = _f64(markers).reshape(-1, 3), _f64(K).reshape(9), _f64(D).reshape(-1)
        frames, n, rows, cols, ptr, on_dev, stride, fstride = self._frame_args(frames)
        out = np.zeros(n, RESULT_DTYPE)
        rc = self._lib.mpe_estimate_batch_wide(self._h, C.c_void_p(ptr), n, rows, cols, stride, fstride, on_dev,
                                               _dp(markers), len(markers), _dp(K), _dp(D), len(D), C.byref(params),
                                               C.c_void_p(out.ctypes.data))
        self._check(rc, "mpe_estimate_batch_wide")
        return out

    def vote_batch_wide(self, dets, markers, K, tol):
        """mpe_vote_batch_wide: dets a list of (n_i, 2) arrays, n_i <= WIDE_DETECTIONS.  -> list of (n_i, n_markers)
        uint32 histograms."""
        markers, K = _f64(markers).reshape(-1, 3), _f64(K).reshape(9)
        buf, nd = self._pack_dets_wide(dets)
        n = len(nd)
        hist = np.zeros((n, WIDE_DETECTIONS, MAX_MARKERS), np.uint32)
        rc = self._lib.mpe_vote_batch_wide(self._h, _dp(buf), nd.ctypes.data_as(C.POINTER(C.c_int)), n, _dp(markers),
                                           len(markers), _dp(K), float(tol), hist.ctypes.data_as(C.POINTER(C.c_uint32)))
        self._check(rc, "mpe_vote_batch_wide")
        return [hist[i, :nd[i], :len(markers)].copy() for i in range(n)]

    def solve_bruteforce_batch_wide(self, dets, markers, K, params):
        """mpe_solve_bruteforce_batch_wide: dets a list of (n_i, 2) arrays, n_i <= WIDE_DETECTIONS.
        -> (records [RESULT_DTYPE] (N), histograms (N, WIDE_DETECTIONS, MAX_MARKERS) uint32, correspondences
        (N, MAX_MARKERS, 2) uint32 — rows (marker, detection), the detection's 1-based index in its set)."""
        markers, K = _f64(markers).reshape(-1, 3), _f64(K).reshape(9)
        buf, nd = self._pack_dets_wide(dets)
        n = len(nd)
        rec = np.zeros(n, RESULT_DTYPE)
        hist = np.zeros((n, WIDE_DETECTIONS, MAX_MARKERS), np.uint32)
        corr = np.zeros((n, MAX_MARKERS, 2), np.uint32)
        up = C.POINTER(C.c_uint32)
        rc = self._lib.mpe_solve_bruteforce_batch_wide(self._h, _dp(buf), nd.ctypes.data_as(C.POINTER(C.c_int)), n,
                                                       _dp(markers), len(markers), _dp(K), C.byref(params),
                                                       C.c_void_p(rec.ctypes.data), hist.ctypes.data_as(up),
                                                       corr.ctypes.data_as(up))
        self._check(rc, "mpe_solve_bruteforce_batch_wide")
        return rec, hist, corr

    def solve_bruteforce_batch_setups(self, dets, setups, item_setup):
        """mpe_solve_bruteforce_batch_setups: dets a list of (n_i, 2) arrays; setups a list of (markers, K, D, params)
        as for track_step_batch (D is not read); item_setup the set-up of every item, or None with one set-up.
        -> (records, histograms, correspondences) as solve_bruteforce_batch, in item order."""
        keep = []
        su = (TrackSetup * len(setups))()
        for s, (markers, K, D, params) in enumerate(setups):
            markers, K, D = _f64(markers).reshape(-1, 3), _f64(K).reshape(9), _f64(D).reshape(-1)
            keep += [markers, K, D, params]
            su[s] = TrackSetup(C.addressof(params), K.ctypes.data, D.ctypes.data if len(D) else None, len(D),
                               markers.ctypes.data, len(markers))
        buf, nd = self._pack_dets(dets)
        n = len(nd)
        idx = None if item_setup is None else (C.c_int * n)(*[int(v) for v in item_setup])
        rec = np.zeros(n, RESULT_DTYPE)
        hist = np.zeros((n, MAX_DETECTIONS, MAX_MARKERS), np.uint32)
        corr = np.zeros((n, MAX_MARKERS, 2), np.uint32)
        up = C.POINTER(C.c_uint32)
        rc = self._lib.mpe_solve_bruteforce_batch_setups(self._h, _dp(buf), nd.ctypes.data_as(C.POINTER(C.c_int)), idx, n,
                                                         su, len(setups), C.c_void_p(rec.ctypes.data),
                                                         hist.ctypes.data_as(up), corr.ctypes.data_as(up))
        self._check(rc, "mpe_solve_bruteforce_batch_setups")
        del keep
        return rec, hist, corr

    # ---- setCorrespondences + checkCorrespondences + optimiseAndUpdatePose ----------------------
    def check_and_refine(self, det, markers, K, params, corr):
        det = _f64(det).reshape(-1, 2)
        markers = _f64(markers).reshape(-1, 3)
        K = _f64(K).reshape(9)
        corr = np.ascontiguousarray(corr, np.uint32).reshape(-1, 2)
        res = MpeResult()
        rc = self._lib.mpe_check_and_refine(self._h, _dp(det), len(det), _dp(markers), len(markers), _dp(K),
                                            C.byref(params), corr.ctypes.data_as(C.POINTER(C.c_uint32)), len(corr),
                                            C.byref(res))
        self._check(rc, "mpe_check_and_refine")
        return dict(status=res.status, T=np.array(res.T).reshape(4, 4), cov=np.array(res.cov).reshape(6, 6),
                    n_corr=res.n_corr, gn_iterations=res.gn_iterations)

    def check_correspondences(self, det, markers, K, params, corr):
        """checkCorrespondences alone -> (ok, unrefined T)."""
        det = _f64(det).reshape(-1, 2)
        markers = _f64(markers).reshape(-1, 3)
        K = _f64(K).reshape(9)
        corr = np.ascontiguousarray(corr, np.uint32).reshape(-1, 2)
        res = MpeResult()
        rc = self._lib.mpe_check_correspondences(self._h, _dp(det), len(det), _dp(markers), len(markers), _dp(K),
                                                 C.byref(params), corr.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 len(corr), C.byref(res))
        self._check(rc, "mpe_check_correspondences")
        return res.status == 0, np.array(res.T).reshape(4, 4)

    def optimise_pose(self, det, markers, K, params, corr, T_init):
        """optimisePose alone from T_init -> dict(status, T, cov, gn_iterations)."""
        det = _f64(det).reshape(-1, 2)
        markers = _f64(markers).reshape(-1, 3)
        K = _f64(K).reshape(9)
        T0 = _f64(T_init).reshape(16)
        corr = np.ascontiguousarray(corr, np.uint32).reshape(-1, 2)
        res = MpeResult()
        rc = self._lib.mpe_optimise_pose(self._h, _dp(det), len(det), _dp(markers), len(markers), _dp(K),
                                         C.byref(params), corr.ctypes.data_as(C.POINTER(C.c_uint32)), len(corr),
                                         _dp(T0), C.byref(res))
        self._check(rc, "mpe_optimise_pose")
        return dict(status=res.status, T=np.array(res.T).reshape(4, 4), cov=np.array(res.cov).reshape(6, 6),
                    gn_iterations=res.gn_iterations)

    def rig_optimise_pose_batch(self, cameras, problems, T_init):
        """mpe_rig_optimise_pose_batch: the joint Gauss-Newton of a rig's cameras, a batch of problems over ONE rig in
        one launch.  cameras: a list of (K 3x3, T_cam_rig 4x4, camera <- rig); problems: a list of row lists, a row =
        (camera index, marker xyz, undistorted pixel uv), in summation order; T_init: (n, 4, 4), rig <- marker frame.
        -> records [RESULT_DTYPE] (n): T, cov (left twist in the rig frame), status, gn_iterations, n_corr = rows,
        n_det = cameras with a row."""
        cams = (MpeRigCamera * max(1, len(cameras)))()
        for c, (K, E) in zip(cams, cameras):
            c.K[:] = _f64(K).reshape(9)
            c.T_cam_rig[:] = _f64(E).reshape(16)
        n = len(problems)
        begin = np.zeros(n + 1, np.int32)
        begin[1:] = np.cumsum([len(rows) for rows in problems])
        flat = [r for rows in problems for r in rows]
        cam = np.ascontiguousarray([r[0] for r in flat], np.int32).reshape(-1)
        xyz = _f64([r[1] for r in flat]).reshape(-1, 3)
        uv = _f64([r[2] for r in flat]).reshape(-1, 2)
        T0 = _f64(T_init).reshape(-1, 16)
        assert len(T0) == n
        rec = np.zeros(n, RESULT_DTYPE)
        ip = C.POINTER(C.c_int)
        rc = self._lib.mpe_rig_optimise_pose_batch(self._h, cams, len(cameras), begin.ctypes.data_as(ip),
                                                   cam.ctypes.data_as(ip), _dp(xyz), _dp(uv), n, _dp(T0), rec.ctypes.data)
        self._check(rc, "mpe_rig_optimise_pose_batch")
        return rec

    def rig_track_batch(self, cameras, markers, detections, T_pred, match_tol, accept_tol, **options):
        """mpe_rig_track_batch: the partial-view tracking step of a rig, a batch of problems over ONE rig and ONE marker
        set in one launch.  cameras: a list of (K 3x3, T_cam_rig 4x4); markers (n_mk, 3); detections: per problem a
        list of n_cam arrays (k, 2) of undistorted pixels (k = 0 .. 64); T_pred (n, 4, 4), rig <- marker frame;
        match_tol / accept_tol: a scalar or n_cam values; options: max_rounds, min_rows, min_markers.
        -> (records [RESULT_DTYPE] (n), match (n, n_cam, n_mk) uint32 — the 1-based detection of (camera, marker)'s row,
        0 none —, info [RIG_TRACK_INFO_DTYPE] (n))."""
        n_cam, n = len(cameras), len(detections)
        cams = pack_rig_cameras(cameras)
        mk = _f64(markers).reshape(-1, 3)
        lists = [_f64(d).reshape(-1, 2) for dets in detections for d in dets]
        assert len(lists) == n * n_cam
        begin = np.zeros(n * n_cam + 1, np.int32)
        begin[1:] = np.cumsum([len(d) for d in lists])
        xy = _f64(np.concatenate(lists) if lists else np.zeros((0, 2))).reshape(-1, 2)
        T0 = _f64(T_pred).reshape(-1, 16)
        assert len(T0) == n
        tm = _f64(np.broadcast_to(_f64(match_tol), (n_cam,)))
        ta = _f64(np.broadcast_to(_f64(accept_tol), (n_cam,)))
        rec = np.zeros(n, RESULT_DTYPE)
        match = np.zeros((n, n_cam, len(mk)), np.uint32)
        info = np.zeros(n, RIG_TRACK_INFO_DTYPE)
        rc = self._lib.mpe_rig_track_batch(self._h, cams, n_cam, _dp(mk), len(mk), begin.ctypes.data_as(C.POINTER(C.c_int)),
                                           _dp(xy), _dp(tm), _dp(ta), n, _dp(T0), rig_track_options(self._lib, options),
                                           rec.ctypes.data, match.ctypes.data, info.ctypes.data)
        self._check(rc, "mpe_rig_track_batch")
        return rec, match, info

    def rig_init_batch(self, cameras, markers, detections, vote_tol, accept_tol, **options):
        """mpe_rig_init_batch: a body found with the whole rig (no predicted pose; one camera must see three blobs), a
        batch of problems over ONE rig and ONE marker set.  cameras, markers, detections as rig_track_batch takes them;
        vote_tol / accept_tol: a scalar or n_cam values; options: max_rounds, min_rows, min_markers, min_margin.
        -> (records [RESULT_DTYPE] (n), match (n, n_cam, n_mk) uint32, info [RIG_INIT_INFO_DTYPE] (n))."""
        n_cam, n = len(cameras), len(detections)
        cams = pack_rig_cameras(cameras)
        mk = _f64(markers).reshape(-1, 3)
        lists = [_f64(d).reshape(-1, 2) for dets in detections for d in dets]
        assert len(lists) == n * n_cam
        begin = np.zeros(n * n_cam + 1, np.int32)
        begin[1:] = np.cumsum([len(d) for d in lists])
        xy = _f64(np.concatenate(lists) if lists else np.zeros((0, 2))).reshape(-1, 2)
        tv = _f64(np.broadcast_to(_f64(vote_tol), (n_cam,)))
        ta = _f64(np.broadcast_to(_f64(accept_tol), (n_cam,)))
        rec = np.zeros(n, RESULT_DTYPE)
        match = np.zeros((n, n_cam, len(mk)), np.uint32)
        info = np.zeros(n, RIG_INIT_INFO_DTYPE)
        rc = self._lib.mpe_rig_init_batch(self._h, cams, n_cam, _dp(mk), len(mk), begin.ctypes.data_as(C.POINTER(C.c_int)),
                                          _dp(xy), _dp(tv), _dp(ta), n, rig_init_options(self._lib, options),
                                          rec.ctypes.data, match.ctypes.data, info.ctypes.data)
        self._check(rc, "mpe_rig_init_batch")
        return rec, match, info

    def rig_init_bodies_batch(self, cameras, bodies, detections, vote_tol, accept_tol, claimed=None, find=None):
        """mpe_rig_init_bodies_batch: several bodies found in one frame, body after body, each in the detections the
        earlier ones left; one device submission.  cameras, detections, vote_tol / accept_tol as rig_init_batch takes
        them; bodies: a list of marker sets (n_mk x 3) or of (markers, options) with options a dict over the bodies'
        defaults (max_rounds, min_rows, min_markers, min_margin) or None; claimed (optional): per problem, per camera a
        flag per detection (non-zero: available to no body); find (optional): (n, n_bodies) flags.
        -> (records [RESULT_DTYPE] (n, n_bodies), match (n, n_bodies, n_cam, MAX_MARKERS) uint32, info
        [RIG_INIT_INFO_DTYPE] (n, n_bodies), owner: per problem, per camera an int8 per detection: -1 free, -2 claimed
        at entry, else the body)."""
        n_cam, n, n_b = len(cameras), len(detections), len(bodies)
        cams = pack_rig_cameras(cameras)
        packed, keep = pack_rig_bodies(self._lib, bodies, n_cam)
        lists = [_f64(d).reshape(-1, 2) for dets in detections for d in dets]
        assert len(lists) == n * n_cam
        begin = np.zeros(n * n_cam + 1, np.int32)
        begin[1:] = np.cumsum([len(d) for d in lists])
        xy = _f64(np.concatenate(lists) if lists else np.zeros((0, 2))).reshape(-1, 2)
        cl = None
        if claimed is not None:
            flags = [np.asarray(f).reshape(-1) != 0 for fl in claimed for f in fl]
            assert [len(f) for f in flags] == [len(d) for d in lists]
            cl = np.ascontiguousarray(np.concatenate(flags) if flags else np.zeros(0), np.uint8)
        fi = None if find is None else np.ascontiguousarray(np.asarray(find).reshape(n, n_b) != 0, np.uint8)
        tv = _f64(np.broadcast_to(_f64(vote_tol), (n_cam,)))
        ta = _f64(np.broadcast_to(_f64(accept_tol), (n_cam,)))
        rec = np.zeros((n, n_b), RESULT_DTYPE)
        match = np.zeros((n, n_b, n_cam, MAX_MARKERS), np.uint32)
        info = np.zeros((n, n_b), RIG_INIT_INFO_DTYPE)
        owner = np.full(len(xy), -1, np.int8)
        rc = self._lib.mpe_rig_init_bodies_batch(self._h, cams, n_cam, packed, n_b, begin.ctypes.data_as(C.POINTER(C.c_int)),
                                                 _dp(xy), None if cl is None else cl.ctypes.data,
                                                 None if fi is None else fi.ctypes.data, _dp(tv), _dp(ta), n,
                                                 rec.ctypes.data, match.ctypes.data, info.ctypes.data, owner.ctypes.data)
        del keep
        self._check(rc, "mpe_rig_init_bodies_batch")
        own = [[owner[begin[i * n_cam + c]:begin[i * n_cam + c + 1]].copy() for c in range(n_cam)] for i in range(n)]
        return rec, match, info, own

    def rig_calibrate(self, cameras, views, T_views, reference_camera=0, max_iterations=50, step_tolerance=1e-10):
        """mpe_rig_calibrate: the extrinsics of a rig from a recorded sequence of ONE body (a bundle adjustment on the
        device over the extrinsics of all cameras but reference_camera and one pose per view).  cameras: a list of
        (K 3x3, T_cam_rig 4x4 camera <- rig, the START value); views: a list of row lists, a row = (camera index, marker
        xyz, undistorted pixel uv), any camera order; T_views: (n, 4, 4) start poses, rig <- marker frame.
        -> dict(T_cam_rig (n_cam, 4, 4), T_views (n, 4, 4), cov (n_cam, 6, 6), view_used (n) bool, report dict,
        ok): ok False (report status 1) hands every extrinsic and pose back as given."""
        cams, begin, cam, xyz, uv = pack_rig_views(cameras, views)
        n, n_cam = len(views), len(cameras)
        T0 = _f64(T_views).reshape(-1, 16)
        assert len(T0) == n
        opt = MpeRigCalibrationOptions(int(reference_camera), int(max_iterations), float(step_tolerance))
        E = np.zeros((max(n_cam, 1), 4, 4))
        T = np.zeros((max(n, 1), 4, 4))
        cov = np.zeros((max(n_cam, 1), 6, 6))
        used = np.zeros(max(n, 1), np.int32)
        rep = MpeRigCalibrationReport()
        ip = C.POINTER(C.c_int)
        rc = self._lib.mpe_rig_calibrate(self._h, cams, n_cam, begin.ctypes.data_as(ip), cam.ctypes.data_as(ip), _dp(xyz),
                                         _dp(uv), n, _dp(T0), C.byref(opt), _dp(E), _dp(T), _dp(cov), used.ctypes.data_as(ip),
                                         C.byref(rep))
        self._check(min(rc, 0), "mpe_rig_calibrate")
        return dict(T_cam_rig=E[:n_cam], T_views=T[:n], cov=cov[:n_cam], view_used=used[:n].astype(bool),
                    report=rig_calibration_report_dict(rep, n_cam), ok=rc == 1)

    def body_calibrate(self, cameras, views, markers, T_views, scale=-1, max_iterations=50, step_tolerance=1e-10):
        """mpe_body_calibrate: the LED positions of ONE body from a recorded sequence (a bundle adjustment on the device
        over the free markers and one pose per view; the extrinsics are fixed).  cameras: a list of (K 3x3, T_cam_rig
        4x4 camera <- rig; a single camera: the identity); views: a list of row lists, a row = (camera index, marker
        INDEX, undistorted pixel uv), any order; markers: (n, 3) START positions; T_views: (n_views, 4, 4) start poses,
        rig <- marker frame; scale: -1 auto, 0 free, 1 held.
        -> dict(markers (n, 3), T_views (n_views, 4, 4), cov (n, 3, 3), view_used (n_views) bool, report dict, ok): ok
        False (report status 1) hands every marker and pose back as given."""
        cams, begin, cam, mk_idx, uv = pack_body_views(cameras, views)
        n, n_cam = len(views), len(cameras)
        mk = _f64(markers).reshape(-1, 3)
        T0 = _f64(T_views).reshape(-1, 16)
        assert len(T0) == n
        opt = MpeBodyCalibrationOptions(int(scale), int(max_iterations), float(step_tolerance))
        P = np.zeros((max(len(mk), 1), 3))
        T = np.zeros((max(n, 1), 4, 4))
        cov = np.zeros((max(len(mk), 1), 3, 3))
        used = np.zeros(max(n, 1), np.int32)
        rep = MpeBodyCalibrationReport()
        ip = C.POINTER(C.c_int)
        rc = self._lib.mpe_body_calibrate(self._h, cams, n_cam, _dp(mk), len(mk), begin.ctypes.data_as(ip),
                                          cam.ctypes.data_as(ip), mk_idx.ctypes.data_as(ip), _dp(uv), n, _dp(T0),
                                          C.byref(opt), _dp(P), _dp(T), _dp(cov), used.ctypes.data_as(ip), C.byref(rep))
        self._check(min(rc, 0), "mpe_body_calibrate")
        return dict(markers=P[:len(mk)], T_views=T[:n], cov=cov[:len(mk)], view_used=used[:n].astype(bool),
                    report=body_calibration_report_dict(rep, len(mk)), ok=rc == 1)

    # ---- one tracked frame: findLeds(ROI) + findCorrespondences + checkCorrespondences + optimisePose ----
    def track_step(self, img, roi, params, K, D, markers, predicted_px):
        img = np.ascontiguousarray(img, np.uint8)
        markers = _f64(markers).reshape(-1, 3)
        K = _f64(K).reshape(9)
        D = _f64(D).reshape(-1)
        pred = _f64(predicted_px).reshape(-1, 2)
        assert len(pred) == len(markers)
        det = MpeDetections()
        corr = np.zeros((MAX_MARKERS, 2), np.uint32)
        res = MpeResult()
        rc = self._lib.mpe_track_step(self._h, C.c_void_p(img.ctypes.data), img.shape[0], img.shape[1],
                                      C.c_size_t(img.strides[0]), int(roi[0]), int(roi[1]), int(roi[2]), int(roi[3]),
                                      C.byref(params), _dp(K), _dp(D), len(D), _dp(markers), len(markers), _dp(pred),
                                      C.byref(det), C.c_void_p(corr.ctypes.data), C.byref(res))
        self._check(rc, "mpe_track_step")
        n = max(det.n, 0)
        return dict(status=res.status, T=np.array(res.T).reshape(4, 4), cov=np.array(res.cov).reshape(6, 6),
                    n_corr=res.n_corr, corr=corr[:max(res.n_corr, 0)].copy(), det_status=det.status,
                    undist=np.array(det.undist_xy[:2 * n]).reshape(-1, 2), gn_iterations=res.gn_iterations)

    # ---- one lock-step time step of N streams: mpe_track_step_batch_setups[_device] ----------------------
    def _track_step_batch(self, entry, ptrs, rows, cols, stride, rois, predicted_px, setups, item_setup, enc=(),
                          formats=None):
        n = len(ptrs)
        keep = []
        su = (TrackSetup * len(setups))()
        for s, (markers, K, D, params) in enumerate(setups):
            markers, K, D = _f64(markers).reshape(-1, 3), _f64(K).reshape(9), _f64(D).reshape(-1)
            keep += [markers, K, D, params]
            su[s] = TrackSetup(C.addressof(params), K.ctypes.data, D.ctypes.data if len(D) else None, len(D),
                               markers.ctypes.data, len(markers))
        items = (TrackItem * n)()
        for i in range(n):
            pred = None if predicted_px[i] is None else _f64(predicted_px[i]).reshape(-1, 2)
            keep.append(pred)
            items[i] = TrackItem(ptrs[i], *[int(v) for v in rois[i]], None if pred is None else pred.ctypes.data)
        idx = None if item_setup is None else (C.c_int * n)(*[int(v) for v in item_setup])
        wide = entry == "mpe_track_step_batch_wide"
        dets = np.zeros(n, DETECTIONS_WIDE_DTYPE if wide else DETECTIONS_DTYPE)
        corr = np.zeros((n, MAX_MARKERS, 2), np.uint32)
        res = np.zeros(n, RESULT_DTYPE)
        # (formats: (item_format, format table, frames_on_device) in place of one shape, stride and encoding)
        shape = (n, rows, cols, C.c_size_t(stride)) + tuple(enc) if formats is None else \
            (formats[0], n, formats[1], len(formats[1]), formats[2])
        rc = getattr(self._lib, entry)(self._h, items, idx, *shape, su, len(setups), C.c_void_p(dets.ctypes.data),
                                       C.c_void_p(corr.ctypes.data), C.c_void_p(res.ctypes.data))
        self._check(rc, entry)
        return dets, corr, res

    def track_step_batch(self, imgs, rois, predicted_px, setups, item_setup):
        """mpe_track_step_batch_setups: one time step of N streams, frames on the host.  imgs: N (rows, cols) uint8
        arrays of one shape and row stride; rois: N x (x, y, w, h); predicted_px: per stream (n_markers, 2) or None
        (detection only); setups: list of (markers, K, D, params); item_setup: the set-up of every stream.
        -> (detections [DETECTIONS_DTYPE] (N), correspondences (N, MAX_MARKERS, 2) uint32, records [RESULT_DTYPE] (N))."""
        rows, cols = imgs[0].shape
        stride = imgs[0].strides[0]
        assert all(im.dtype == np.uint8 and im.shape == (rows, cols) and im.strides == (stride, 1) for im in imgs)
        return self._track_step_batch("mpe_track_step_batch_setups", [im.ctypes.data for im in imgs], rows, cols, stride,
                                      rois, predicted_px, setups, item_setup)

    def track_step_batch_device(self, imgs, rois, predicted_px, setups, item_setup=None, encoding="mono8", big_endian=False):
        """mpe_track_step_batch_setups_device: track_step_batch for frames in device memory.  imgs: a list of N
        (rows, cols) torch uint8 CUDA tensors on this handle's device (any common row stride), or one (N, rows, cols)
        tensor; item_setup None: one set-up for all.  Same records as track_step_batch over the same frames.
        encoding other than "mono8" (ENCODINGS; big_endian for "mono16"): mpe_track_step_batch_setups_device_encoded
        over frames in that encoding — (rows, cols, bytes per pixel) uint8 or, mono16, (rows, cols) uint16 / int16
        tensors; rois stay in pixels.  Same records as the mono8 call over the frames after convert_to_mono8."""
        keep, ptrs, (rows, cols), (stride, _) = _device_images(imgs, 0, encoding)
        if encoding == "mono8":
            out = self._track_step_batch("mpe_track_step_batch_setups_device", list(ptrs), rows, cols, stride, rois,
                                         predicted_px, setups, item_setup)
        else:
            out = self._track_step_batch("mpe_track_step_batch_setups_device_encoded", list(ptrs), rows, cols, stride, rois,
                                         predicted_px, setups, item_setup, _enc_args(encoding, big_endian))
        del keep
        return out

    def track_step_batch_formats(self, imgs, rois, predicted_px, setups, item_setup=None, formats=None, item_format=None):
        """mpe_track_step_batch_formats: one time step of N streams whose images may differ in size, row stride and
        encoding, in ONE submission.  imgs: N numpy arrays (host frames, mono8) or N torch CUDA tensors on this handle's
        device, of any shapes; rois in pixels of the item's own image; formats: None (mono8 formats read off the arrays),
        or per item an encoding name, (name, big_endian) or an ImageFormat — equal ones share an entry of the format
        table.  With item_format, formats is the table itself (ImageFormat entries) and item_format[i] item i's index.
        item_setup None: one set-up for all.  -> (detections, correspondences, records) as track_step_batch: every item's
        are those of track_step_batch / track_step_batch_device over the items of its format alone."""
        if item_format is None:
            on_device, ptrs, fmts, _ = _stream_formats(imgs, 0, formats)
            table, index = [], {}
            item_format = [index.setdefault(f.key(), len(index)) for f in fmts]
            for f, k in zip(fmts, item_format):
                if k == len(table):
                    table.append(f)
        else:
            on_device, ptrs, _, _ = _stream_formats(imgs, 0, [formats[k] for k in item_format])
            table = list(formats)
        n = len(ptrs)
        ifmt = None if len(table) == 1 else (C.c_int * n)(*[int(k) for k in item_format])
        return self._track_step_batch("mpe_track_step_batch_formats", ptrs, 0, 0, 0, rois, predicted_px, setups, item_setup,
                                      formats=(ifmt, (ImageFormat * len(table))(*table), on_device))

    def track_step_batch_wide(self, imgs, rois, predicted_px, setups, item_setup=None, encoding="mono8", big_endian=False):
        """mpe_track_step_batch_wide: track_step_batch / track_step_batch_device with records of WIDE_DETECTIONS points
        (synchronous).  imgs: host frames as track_step_batch takes them (numpy, mono8), or device frames as
        track_step_batch_device takes them (torch CUDA tensors, any of ENCODINGS).  -> (detections
        [DETECTIONS_WIDE_DTYPE] (N), correspondences (N, MAX_MARKERS, 2) uint32 with detection indices 1 .. 256,
        records [RESULT_DTYPE] (N)); for a stream of at most MAX_DETECTIONS detections, the narrow entries' records."""
        on_device = _is_torch(imgs) or _is_torch(imgs[0])
        if on_device:
            keep, ptrs, (rows, cols), (stride, _) = _device_images(imgs, 0, encoding)
            ptrs = list(ptrs)
        else:
            if encoding != "mono8":
                raise MpeError("host frames are mono8 (the encodings are decoded from device frames)")
            rows, cols = imgs[0].shape
            stride = imgs[0].strides[0]
            assert all(im.dtype == np.uint8 and im.shape == (rows, cols) and im.strides == (stride, 1) for im in imgs)
            keep, ptrs = imgs, [im.ctypes.data for im in imgs]
        out = self._track_step_batch("mpe_track_step_batch_wide", ptrs, rows, cols, stride, rois, predicted_px, setups,
                                     item_setup, (int(on_device),) + _enc_args(encoding, big_endian))
        del keep
        return out

    # ---- static primitives, batched ----------------------------------------------------------------
    def p3p_batch(self, fv, wp):
        """fv, wp: (n,3,3), ROWS = bearings / world points.  -> (status (n,), solutions (n,4,3,4) [R|C])."""
        fv = _f64(fv).reshape(-1, 9)
        wp = _f64(wp).reshape(-1, 9)
        n = len(fv)
        sol = np.zeros((n, 4, 3, 4))
        st = np.zeros(n, np.int32)
        self._check(self._lib.mpe_p3p_batch(self._h, _dp(fv), _dp(wp), n, _dp(sol), C.c_void_p(st.ctypes.data)),
                    "mpe_p3p_batch")
        return st, sol

    def solve_quartic_batch(self, factors, variant=0):
        f = _f64(factors).reshape(-1, 5)
        r = np.zeros((len(f), 4))
        self._check(self._lib.mpe_solve_quartic_batch(self._h, _dp(f), len(f), int(variant), _dp(r)),
                    "mpe_solve_quartic_batch")
        return r

    def ddmath_batch(self, which, a, b=None):
        """Primitive `which` of csrc/mpe_ddmath.h (selectors: include/mpe.h) at the pairs (a[i], b[i]); b defaults to
        a.  -> (n, 2) = (out0, out1)."""
        a = _f64(a).reshape(-1)
        b = a if b is None else _f64(b).reshape(-1)
        if len(b) != len(a):
            raise MpeError("a and b differ in length")
        out = np.zeros((len(a), 2))
        self._check(self._lib.mpe_ddmath_batch(self._h, int(which), _dp(a), _dp(b), len(a), _dp(out)), "mpe_ddmath_batch")
        return out

    # ---- estimateBodyPose on a fresh estimator per frame -------------------------------------
    def estimate_batch(self, frames, markers, K, D, params):
        """frames: numpy (n,rows,cols) uint8 on the host, or a torch uint8 CUDA tensor (n,rows,cols)."""
        markers = _f64(markers).reshape(-1, 3)
        K = _f64(K).reshape(9)
        D = _f64(D).reshape(-1)
        if _is_torch(frames):
            assert frames.is_cuda and frames.is_contiguous() and frames.dtype.is_floating_point is False
            n, rows, cols = frames.shape
            ptr, on_dev, stride, fstride = frames.data_ptr(), 1, cols, rows * cols
        else:
            frames = np.ascontiguousarray(frames, np.uint8)
            n, rows, cols = frames.shape
            ptr, on_dev, stride, fstride = frames.ctypes.data, 0, frames.strides[1], frames.strides[0]
        out = np.zeros(n, RESULT_DTYPE)
        rc = self._lib.mpe_estimate_batch(self._h, C.c_void_p(ptr), n, rows, cols, stride, fstride, on_dev,
                                          _dp(markers), len(markers), _dp(K), _dp(D), len(D), C.byref(params),
                                          C.c_void_p(out.ctypes.data))
        self._check(rc, "mpe_estimate_batch")
        return out

    def estimate_batch_device(self, d_frames_ptr, n, rows, cols, markers, K, D, params, d_results_ptr):
        """Fully asynchronous: device frames in, device results out, kernels only."""
        markers = _f64(markers).reshape(-1, 3)
        K = _f64(K).reshape(9)
        D = _f64(D).reshape(-1)
        rc = self._lib.mpe_estimate_batch_device(self._h, C.c_void_p(d_frames_ptr), n, rows, cols, _dp(markers),
                                                 len(markers), _dp(K), _dp(D), len(D), C.byref(params),
                                                 C.c_void_p(d_results_ptr))
        self._check(rc, "mpe_estimate_batch_device")

    def convert_to_mono8(self, src, encoding, big_endian=False):
        """mpe_convert_to_mono8 for a batch: src (n, rows, cols[, channels]) uint8 / (n, rows, cols) uint16 numpy array
        (host) or torch CUDA tensor; encoding: one of ENCODINGS — (n, rows, cols) uint8 for mono8 and the Bayer patterns,
        (n, rows, cols, 2) uint8 for yuv422 / yuv422_yuy2.  A device source whose pixels are contiguous within a row is
        read in place, whatever its row stride, frame stride and storage offset are.
        -> (n, rows, cols) uint8, numpy for a host source, a torch CUDA tensor for a device source."""
        enc = ENCODINGS[encoding]
        if _is_torch(src):
            import torch
            n, rows, cols = src.shape[:3]
            es = src.element_size()
            bpp = es * (src.shape[3] if src.dim() == 4 else 1)
            dense = src.stride(-1) == 1 and (src.dim() == 3 or src.stride(2) == src.shape[3])
            # (the stride of a dimension of size 1 says nothing)
            stride = src.stride(1) * es if rows > 1 else cols * bpp
            fstride = src.stride(0) * es if n > 1 else rows * stride
            if not (dense and stride >= cols * bpp and fstride >= rows * stride):
                src = src.contiguous()
                stride, fstride = cols * bpp, rows * cols * bpp
            dst = torch.empty((n, rows, cols), dtype=torch.uint8, device=src.device)
            rc = self._lib.mpe_convert_to_mono8(self._h, C.c_void_p(src.data_ptr()), 1, enc, int(bool(big_endian)), n, rows,
                                                cols, C.c_size_t(stride), C.c_size_t(fstride), C.c_void_p(dst.data_ptr()), 1)
            self._check(rc, "mpe_convert_to_mono8")
            self.synchronize()
            return dst
        src = np.ascontiguousarray(src)
        n, rows, cols = src.shape[:3]
        raw = src.view(np.uint8).reshape(n, rows, -1)
        dst = np.zeros((n, rows, cols), np.uint8)
        rc = self._lib.mpe_convert_to_mono8(self._h, C.c_void_p(raw.ctypes.data), 0, enc, int(bool(big_endian)), n, rows, cols,
                                            C.c_size_t(raw.strides[1]), C.c_size_t(raw.strides[0]),
                                            C.c_void_p(dst.ctypes.data), 0)
        self._check(rc, "mpe_convert_to_mono8")
        return dst

    def estimate_batch_device_submit(self, d_frames_ptr, n, rows, cols, markers, K, D, params, d_results_ptr,
                                     d_next_frames_ptr=0, n_next=0):
        """Streaming variant: enqueue only, no join of the internal side streams; `d_next_frames_ptr` announces the
        frames of the next submission (its first sub-batch is then scanned by this one's last voting launch)."""
        markers = _f64(markers).reshape(-1, 3)
        K = _f64(K).reshape(9)
        D = _f64(D).reshape(-1)
        rc = self._lib.mpe_estimate_batch_device_submit(self._h, C.c_void_p(d_frames_ptr), n, rows, cols, _dp(markers),
                                                        len(markers), _dp(K), _dp(D), len(D), C.byref(params),
                                                        C.c_void_p(d_results_ptr), C.c_void_p(d_next_frames_ptr or None),
                                                        int(n_next))
        self._check(rc, "mpe_estimate_batch_device_submit")

    def stream_next_ready(self, event_ptr):
        """The frames the NEXT _submit announces are final once this hipEvent_t has completed (one-shot)."""
        self._check(self._lib.mpe_stream_next_ready(self._h, C.c_void_p(event_ptr or None)), "mpe_stream_next_ready")

    def stream_drop_prefetch(self):
        """Forget what the last submission scanned ahead: the announced buffer has been rewritten since."""
        self._check(self._lib.mpe_stream_drop_prefetch(self._h), "mpe_stream_drop_prefetch")

    def estimate_batch_device_collect(self, stream_ptr=0):
        """Make `stream_ptr` (0 = the handle's stream) wait for the records of the oldest un-collected submission."""
        self._check(self._lib.mpe_estimate_batch_device_collect(self._h, C.c_void_p(stream_ptr or None)),
                    "mpe_estimate_batch_device_collect")

    # ---- stage level ---------------------------------------------------------------------------
    def detect_batch(self, frames, K, D, params):
        K = _f64(K).reshape(9)
        D = _f64(D).reshape(-1)
        if _is_torch(frames):
            n, rows, cols = frames.shape
            ptr, on_dev, stride, fstride = frames.data_ptr(), 1, cols, rows * cols
        else:
            frames = np.ascontiguousarray(frames, np.uint8)
            n, rows, cols = frames.shape
            ptr, on_dev, stride, fstride = frames.ctypes.data, 0, frames.strides[1], frames.strides[0]
        out = np.zeros(n, DETECTIONS_DTYPE)
        rc = self._lib.mpe_detect_batch(self._h, C.c_void_p(ptr), n, rows, cols, stride, fstride, on_dev, _dp(K),
                                        _dp(D), len(D), C.byref(params), C.c_void_p(out.ctypes.data))
        self._check(rc, "mpe_detect_batch")
        return out

    def vote_batch(self, dets, markers, K, tol):
        """dets: list of (n_i,2) arrays.  -> list of (n_i, n_markers) uint32 histograms."""
        markers = _f64(markers).reshape(-1, 3)
        K = _f64(K).reshape(9)
        n = len(dets)
        buf = np.zeros((n, MAX_DETECTIONS, 2))
        nd = np.zeros(n, np.int32)
        for i, d in enumerate(dets):
            d = _f64(d).reshape(-1, 2)
            nd[i] = len(d)
            buf[i, :len(d)] = d
        hist = np.zeros((n, MAX_DETECTIONS, MAX_MARKERS), np.uint32)
        rc = self._lib.mpe_vote_batch(self._h, _dp(buf), nd.ctypes.data_as(C.POINTER(C.c_int)), n, _dp(markers),
                                      len(markers), _dp(K), float(tol), hist.ctypes.data_as(C.POINTER(C.c_uint32)))
        self._check(rc, "mpe_vote_batch")
        return [hist[i, :nd[i], :len(markers)].copy() for i in range(n)]


    def vote_items(self, det, markers, K, tol, lo, hi):
        """Forensics: the detection set `det` voted len(lo) times, copy i with the hypotheses [lo[i], hi[i]) only
        (flattened index = triple index * P(n_markers,3) + permutation index).  -> (len(lo), n_det, n_markers)."""
        markers = _f64(markers).reshape(-1, 3)
        K = _f64(K).reshape(9)
        det = _f64(det).reshape(-1, 2)
        lo = np.ascontiguousarray(lo, np.int32)
        hi = np.ascontiguousarray(hi, np.int32)
        n = len(lo)
        buf = np.zeros((n, MAX_DETECTIONS, 2))
        buf[:, :len(det)] = det
        nd = np.full(n, len(det), np.int32)
        hist = np.zeros((n, MAX_DETECTIONS, MAX_MARKERS), np.uint32)
        ip = C.POINTER(C.c_int)
        rc = self._lib.mpe_vote_items(self._h, _dp(buf), nd.ctypes.data_as(ip), n, _dp(markers), len(markers), _dp(K),
                                      float(tol), lo.ctypes.data_as(ip), hi.ctypes.data_as(ip),
                                      hist.ctypes.data_as(C.POINTER(C.c_uint32)))
        self._check(rc, "mpe_vote_items")
        return hist[:, :len(det), :len(markers)].copy()


class Tracker:
    """mpe_tracker: one stateful PoseEstimator object (uninitialised branch + tracking path)."""

    def __init__(self, handle, markers, K, D, params):
        self._handle = handle
        self._lib = load_library()
        self._t = C.c_void_p()
        rc = self._lib.mpe_tracker_create(handle._h, C.byref(self._t))
        if rc != 0:
            raise MpeError("mpe_tracker_create failed (%d)" % rc)
        markers = _f64(markers).reshape(-1, 3)
        K = _f64(K).reshape(9)
        D = _f64(D).reshape(-1)
        self.markers, self.K = markers.copy(), K.reshape(3, 3).copy()
        handle._check(self._lib.mpe_tracker_set_markers(self._t, _dp(markers), len(markers)), "mpe_tracker_set_markers")
        handle._check(self._lib.mpe_tracker_set_camera(self._t, _dp(K), _dp(D), len(D)), "mpe_tracker_set_camera")
        self.set_params(params)

    def set_markers(self, markers):
        """setMarkerPositions(): another marker set (what BodyCalibrator.apply hands over)."""
        markers = _f64(markers).reshape(-1, 3)
        self._handle._check(self._lib.mpe_tracker_set_markers(self._t, _dp(markers), len(markers)), "mpe_tracker_set_markers")
        self.markers = markers.copy()

    def set_params(self, params):
        self._handle._check(self._lib.mpe_tracker_set_params(self._t, C.byref(params)), "mpe_tracker_set_params")

    def reset(self):
        self._lib.mpe_tracker_reset(self._t)

    def set_wide_frames(self, on):
        """mpe_tracker_set_wide_frames: frames of 65 .. WIDE_DETECTIONS detections are answered (default off)."""
        self._handle._check(self._lib.mpe_tracker_set_wide_frames(self._t, int(bool(on))), "mpe_tracker_set_wide_frames")

    def estimate(self, img, time):
        img = np.ascontiguousarray(img, np.uint8)
        res = MpeResult()
        info = (C.c_int * 8)()
        rc = self._lib.mpe_tracker_estimate(self._t, img.ctypes.data, img.shape[0], img.shape[1], img.strides[0],
                                            float(time), C.byref(res), info)
        if rc < 0:
            raise MpeError("mpe_tracker_estimate failed (%d): %s" % (rc, self._lib.mpe_last_error(self._handle._h).decode()))
        return dict(updated=bool(rc), T=np.array(res.T).reshape(4, 4), cov=np.array(res.cov).reshape(6, 6),
                    roi=tuple(info[0:4]), it_since_initialized=info[4], n_det=info[5], n_corr=info[6],
                    used_bruteforce=bool(info[7]))

    def correspondences(self):
        """getCorrespondences(): the rows (marker, detection), 1-based, of the last frame that made any -> (n, 2) uint32."""
        n = self._lib.mpe_tracker_get_correspondences(self._t, None, 0)
        corr = np.zeros((max(n, 0), 2), np.uint32)
        self._lib.mpe_tracker_get_correspondences(self._t, corr.ctypes.data_as(C.POINTER(C.c_uint32)), len(corr))
        return corr

    def image_points(self):
        """getImagePoints(): the undistorted detections of the last frame -> (n, 2) float64."""
        n = self._lib.mpe_tracker_get_image_points(self._t, None, 0)
        xy = np.zeros((max(n, 0), 2))
        self._lib.mpe_tracker_get_image_points(self._t, _dp(xy), len(xy))
        return xy

    def run_sequence(self, frames, times):
        """The image-callback loop in C over a recorded sequence (frames (n,rows,cols) uint8, C-contiguous).
        -> (records [RESULT_DTYPE], info (n,8) int32).  ctypes drops the GIL for the duration."""
        frames = np.ascontiguousarray(frames, np.uint8)
        times = _f64(times).reshape(-1)
        n = frames.shape[0]
        rec = np.zeros(n, RESULT_DTYPE)
        info = np.zeros((n, 8), np.int32)
        rc = self._lib.mpe_tracker_run_sequence(self._t, frames.ctypes.data, n, frames.shape[1], frames.shape[2],
                                                frames.strides[1], frames.strides[0], _dp(times), rec.ctypes.data,
                                                info.ctypes.data)
        if rc < 0:
            raise MpeError("mpe_tracker_run_sequence failed (%d): %s"
                           % (rc, self._lib.mpe_last_error(self._handle._h).decode()))
        return rec, info

    def close(self):
        if getattr(self, "_t", None):
            self._lib.mpe_tracker_destroy(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Rig:
    """The cameras of a calibrated rig that see ONE body: a lock-step group of trackers (one per camera, one handle, one
    marker set) plus the extrinsics T_cam_rig (n, 4, 4), camera <- rig, trusted as given.  step() drives the group's
    lock-step entry, then fuses the cameras that updated into one pose, rig <- marker frame, with one covariance
    (mpe_rig_fuse_trackers: the joint Gauss-Newton on the device)."""

    def __init__(self, handle, trackers, T_cam_rig):
        self.handle = handle
        self.trackers = list(trackers)
        self.T_cam_rig = _f64(T_cam_rig).reshape(len(self.trackers), 16)
        self._ts = (C.c_void_p * len(self.trackers))(*[t._t for t in self.trackers])
        self._prev = None  # (rig pose, time) of the previous step when it fused
        self._prev2 = None  # the same of the step before that, when both fused (step(partial=True) predicts from the two)
        self.last_track = self.last_init = None

    def fuse(self, updated=None):
        """mpe_rig_fuse_trackers over the trackers' last frames -> (fused, record [RESULT_DTYPE] (1), rows per camera)."""
        lib, n = self.handle._lib, len(self.trackers)
        rec = np.zeros(1, RESULT_DTYPE)
        rows = np.zeros(n, np.int32)
        upd = None if updated is None else np.ascontiguousarray(updated, np.int32)
        ip = C.POINTER(C.c_int)
        rc = lib.mpe_rig_fuse_trackers(self._ts, n, _dp(self.T_cam_rig), None if upd is None else upd.ctypes.data_as(ip),
                                       rec.ctypes.data, rows.ctypes.data_as(ip))
        if rc < 0:
            raise MpeError("mpe_rig_fuse_trackers failed (%d): %s" % (rc, lib.mpe_last_error(self.handle._h).decode()))
        return bool(rc), rec, rows

    def track(self, T_pred, **options):
        """mpe_rig_track_trackers over the trackers' last frames from the predicted rig pose T_pred (4x4, rig <- marker
        frame): every camera's image points count, whether or not its own tracker solved the frame.  options:
        max_rounds, min_rows, min_markers.  -> (pose found, record [RESULT_DTYPE] (1), match (n, n_markers) uint32,
        info [RIG_TRACK_INFO_DTYPE] (1))."""
        lib, n = self.handle._lib, len(self.trackers)
        rec = np.zeros(1, RESULT_DTYPE)
        match = np.zeros((n, len(self.trackers[0].markers)), np.uint32)
        info = np.zeros(1, RIG_TRACK_INFO_DTYPE)
        rc = lib.mpe_rig_track_trackers(self._ts, n, _dp(self.T_cam_rig), _dp(_f64(T_pred).reshape(16)),
                                        rig_track_options(lib, options), rec.ctypes.data, match.ctypes.data, info.ctypes.data)
        if rc < 0:
            raise MpeError("mpe_rig_track_trackers failed (%d): %s" % (rc, lib.mpe_last_error(self.handle._h).decode()))
        return bool(rc), rec, match, info

    def init(self, **options):
        """mpe_rig_init_trackers over the trackers' last frames: the body found with the whole rig, without a predicted
        pose (P3P hypotheses from every camera with three image points, support counted in all cameras).  options:
        max_rounds, min_rows, min_markers, min_margin.  -> (pose found, record [RESULT_DTYPE] (1), match (n, n_markers)
        uint32, info [RIG_INIT_INFO_DTYPE] (1))."""
        lib, n = self.handle._lib, len(self.trackers)
        rec = np.zeros(1, RESULT_DTYPE)
        match = np.zeros((n, len(self.trackers[0].markers)), np.uint32)
        info = np.zeros(1, RIG_INIT_INFO_DTYPE)
        rc = lib.mpe_rig_init_trackers(self._ts, n, _dp(self.T_cam_rig), rig_init_options(lib, options), rec.ctypes.data,
                                       match.ctypes.data, info.ctypes.data)
        if rc < 0:
            raise MpeError("mpe_rig_init_trackers failed (%d): %s" % (rc, lib.mpe_last_error(self.handle._h).decode()))
        return bool(rc), rec, match, info

    def predict(self, time):
        """The rig pose the constant-velocity model (predict_pose) gives at `time` from the last two fused steps, the last
        pose itself when only one step fused, None without a previous rig pose."""
        if self._prev is None:
            return None
        if self._prev2 is None or not self._prev[1] > self._prev2[1]:
            return self._prev[0].reshape(4, 4).copy()
        return predict_pose(self._prev[0].reshape(4, 4), self._prev2[0].reshape(4, 4), self._prev[1], self._prev2[1], time)

    def seed(self, seed, rig_pose, time, rig_prev_pose=None, prev_time=0.0):
        """mpe_rig_seed_trackers: the trackers with seed[i] != 0 get their pose from the rig's (host state only)."""
        lib, n = self.handle._lib, len(self.trackers)
        sd = np.ascontiguousarray(seed, np.int32)
        prev = None if rig_prev_pose is None else _dp(_f64(rig_prev_pose).reshape(16))
        rc = lib.mpe_rig_seed_trackers(self._ts, n, _dp(self.T_cam_rig), sd.ctypes.data_as(C.POINTER(C.c_int)),
                                       _dp(_f64(rig_pose).reshape(16)), float(time), prev, float(prev_time))
        if rc < 0:
            raise MpeError("mpe_rig_seed_trackers failed (%d)" % rc)

    def step(self, imgs, times, formats=None, reseed=False, partial=False, init=False):
        """One time step: imgs[i] / times[i] camera i's frame and stamp.  Cameras of one image shape go through
        tracker_estimate_batch_mixed, others (or formats given: as tracker_estimate_batch_formats takes them) through
        tracker_estimate_batch_formats; then the fusion.  reseed: the trackers that did NOT update get the rig's pose
        (and the previous step's, when that step fused), so that their next frame tracks instead of running the brute
        force.  partial: with a rig pose from the previous step, predict it to this step's time (predict()) and track
        the body over ALL cameras' image points (track(): a camera that sees two or three LEDs counts) instead of fusing
        the cameras that solved the frame on their own; without a previous rig pose, or when tracking finds no pose, the
        fusion as ever.  self.last_track = (record, match, info) of the step's track() or None.  init: a step that ends
        with no rig pose — after the fusion, and after the tracking where partial is on — runs init(); a pose found there
        counts as fused (reseed seeds the trackers from it, the next step tracks from it).  self.last_init = (record,
        match, info) of the step's init() or None.
        -> (records (N), info (N, 8), updated (N) — the lock-step entry's, unchanged —, rig record (1), fused)."""
        same = formats is None and not _is_torch(imgs[0]) and len({(np.shape(im), np.asarray(im).strides[0]) for im in imgs}) == 1
        if same:
            rec, info, upd = tracker_estimate_batch_mixed(self.trackers, imgs, times)
        else:
            rec, info, upd = tracker_estimate_batch_formats(self.trackers, imgs, times, formats)
        t = float(np.max(_f64(times)))
        fused, self.last_track = False, None
        if partial and self._prev is not None:
            fused, rig, match, tinfo = self.track(self.predict(t))
            self.last_track = (rig, match, tinfo)
        if not fused:
            fused, rig, _ = self.fuse(upd)
        self.last_init = None
        if init and not fused:
            fused, found, match, iinfo = self.init()
            self.last_init = (found, match, iinfo)
            if fused:
                rig = found
        if reseed and fused and not upd.all():
            prev = self._prev
            self.seed(~upd, rig["T"][0], t, None if prev is None else prev[0], 0.0 if prev is None else prev[1])
        self._prev2 = self._prev if fused else None
        self._prev = (rig["T"][0].copy(), t) if fused else None
        return rec, info, upd, rig, fused


class Bodies:
    """Several bodies in front of one rig (or one camera): trackers[b][c] is body b in camera c, all on one handle;
    T_cam_rig (n_cam, 4, 4), camera <- rig, None for a single camera (the identity).  A tracker's own initialiser sums the
    votes of everything in view into one histogram and mixes the bodies up, so here a body gets its FIRST pose only from
    mpe_rig_init_bodies_trackers, which finds body after body, each in the detections the others left; a pose that a
    tracker's own brute force gave is dropped (the tracker is reset) and the body is searched for with the others'
    points claimed.  Once seeded, a body's trackers follow it in their ROIs as ever."""

    def __init__(self, handle, trackers, T_cam_rig=None):
        self.handle = handle
        self.trackers = [list(ts) for ts in trackers]
        self.n_bodies, self.n_cam = len(self.trackers), len(self.trackers[0])
        assert all(len(ts) == self.n_cam for ts in self.trackers)
        self.T_cam_rig = None if T_cam_rig is None else _f64(T_cam_rig).reshape(self.n_cam, 16)
        assert self.T_cam_rig is not None or self.n_cam == 1
        self._flat = [t for ts in self.trackers for t in ts]
        self._ts = (C.c_void_p * len(self._flat))(*[t._t for t in self._flat])
        self._rigs = [Rig(handle, ts, np.eye(4).reshape(1, 16) if self.T_cam_rig is None else self.T_cam_rig)
                      for ts in self.trackers]
        self.last_init = None  # (records, match, info, owner) of the step's mpe_rig_init_bodies_trackers, or None

    def init(self, find, updated, claim_radius=2.0):
        """mpe_rig_init_bodies_trackers over the trackers' last frames -> (bodies found, records [RESULT_DTYPE]
        (n_bodies), match (n_bodies, n_cam, MAX_MARKERS) uint32, info [RIG_INIT_INFO_DTYPE] (n_bodies), owner: per camera
        an int8 per point of its list — the image points of the first searched body's tracker of that camera)."""
        lib, nb, nc = self.handle._lib, self.n_bodies, self.n_cam
        fi = np.ascontiguousarray(np.asarray(find).reshape(nb) != 0, np.int32)
        up = np.ascontiguousarray(np.asarray(updated).reshape(nb * nc) != 0, np.int32)
        rec = np.zeros(nb, RESULT_DTYPE)
        match = np.zeros((nb, nc, MAX_MARKERS), np.uint32)
        info = np.zeros(nb, RIG_INIT_INFO_DTYPE)
        lens = [0] * nc
        if fi.any():
            b0 = int(np.argmax(fi))
            lens = [len(self.trackers[b0][c].image_points()) for c in range(nc)]
        owner = np.full(max(1, sum(lens)), -1, np.int8)
        ip = C.POINTER(C.c_int)
        rc = lib.mpe_rig_init_bodies_trackers(self._ts, nb, nc, None if self.T_cam_rig is None else _dp(self.T_cam_rig),
                                              fi.ctypes.data_as(ip), up.ctypes.data_as(ip), float(claim_radius),
                                              rec.ctypes.data, match.ctypes.data, info.ctypes.data, owner.ctypes.data)
        if rc < 0:
            raise MpeError("mpe_rig_init_bodies_trackers failed (%d): %s" % (rc, lib.mpe_last_error(self.handle._h).decode()))
        cuts = np.concatenate([[0], np.cumsum(lens)]).astype(int)
        return rc, rec, match, info, [owner[cuts[c]:cuts[c + 1]].copy() for c in range(nc)]

    def step(self, imgs, times, formats=None, claim_radius=2.0):
        """One time step: imgs[c] / times[c] camera c's frame and stamp (formats: as tracker_estimate_batch_formats takes
        them, per camera).  Every body's tracker of camera c gets camera c's image in ONE lock-step call; a body that no
        camera updated while tracking is searched for with the points of the tracked bodies claimed within
        claim_radius pixels, and the found ones are seeded.  self.last_init: what that search returned, or None.
        -> (records [RESULT_DTYPE] (n_bodies): a tracked body's is its tracker's (one camera) or the fusion of its
        cameras', a searched body's is the search's —, info (n_bodies, n_cam, 8) the lock-step entry's, owner: the
        search's owner map per camera, or None)."""
        nb, nc = self.n_bodies, self.n_cam
        flat_imgs = [imgs[c] for _ in range(nb) for c in range(nc)]
        flat_times = [float(_f64(times).reshape(-1)[c]) for _ in range(nb) for c in range(nc)]
        same = formats is None and not _is_torch(imgs[0]) and len({(np.shape(im), np.asarray(im).strides[0]) for im in imgs}) == 1
        if same:
            rec, info, upd = tracker_estimate_batch_mixed(self._flat, flat_imgs, flat_times)
        else:
            fm = None if formats is None else [formats[c] for _ in range(nb) for c in range(nc)]
            rec, info, upd = tracker_estimate_batch_formats(self._flat, flat_imgs, flat_times, fm)
        rec, info = rec.reshape(nb, nc), info.reshape(nb, nc, 8)
        # a camera counts when its tracker followed the body; what its own brute force found may be any body's
        tracked = np.asarray(upd, bool).reshape(nb, nc) & (info[:, :, 7] == 0)
        find = ~tracked.any(axis=1)
        out = np.zeros(nb, RESULT_DTYPE)
        t = float(np.max(_f64(times)))
        for b in range(nb):
            if find[b]:
                continue
            if nc == 1:
                out[b] = rec[b, 0]
            else:
                out[b] = self._rigs[b].fuse(tracked[b])[1][0]
        self.last_init, owner = None, None
        if find.any():
            _, found, match, iinfo, owner = self.init(find, tracked, claim_radius)
            self.last_init = (found, match, iinfo, owner)
            for b in np.nonzero(find)[0]:
                out[b] = found[b]
                if found[b]["status"] == 0:
                    self._rigs[b].seed(np.ones(nc, np.int32), found[b]["T"], t)
                else:
                    for tr in self.trackers[b]:
                        tr.reset()
        return out, info, owner


def pack_rig_cameras(cameras):
    """[(K 3x3, T_cam_rig 4x4)] -> mpe_rig_camera array"""
    cams = (MpeRigCamera * max(1, len(cameras)))()
    for c, (K, E) in zip(cams, cameras):
        c.K[:] = _f64(K).reshape(9)
        c.T_cam_rig[:] = _f64(E).reshape(16)
    return cams


def rig_track_options(lib, options):
    """max_rounds / min_rows / min_markers over the library's defaults -> MpeRigTrackOptions"""
    opt = MpeRigTrackOptions()
    lib.mpe_rig_track_default_options(C.byref(opt))
    for k, v in options.items():
        if k not in ("max_rounds", "min_rows", "min_markers"):
            raise TypeError("unknown option %r" % k)
        setattr(opt, k, int(v))
    return opt


def rig_init_options(lib, options):
    """max_rounds / min_rows / min_markers / min_margin over the library's defaults -> MpeRigInitOptions"""
    opt = MpeRigInitOptions()
    lib.mpe_rig_init_default_options(C.byref(opt))
    for k, v in options.items():
        if k not in ("max_rounds", "min_rows", "min_markers", "min_margin"):
            raise TypeError("unknown option %r" % k)
        setattr(opt, k, int(v))
    return opt


def rig_init_bodies_options(lib, options, n_cameras, n_markers):
    """max_rounds / min_rows / min_markers / min_margin over the bodies' defaults -> MpeRigInitOptions"""
    opt = MpeRigInitOptions()
    lib.mpe_rig_init_bodies_default_options(C.byref(opt), int(n_cameras), int(n_markers))
    for k, v in (options or {}).items():
        if k not in ("max_rounds", "min_rows", "min_markers", "min_margin"):
            raise TypeError("unknown option %r" % k)
        setattr(opt, k, int(v))
    return opt


def pack_rig_bodies(lib, bodies, n_cameras):
    """[markers (n_mk x 3) | (markers, options dict or None)] -> (mpe_rig_body array, what it points to: keep it alive)"""
    arr = (MpeRigBody * max(1, len(bodies)))()
    keep = []
    for a, body in zip(arr, bodies):
        markers, options = body if isinstance(body, tuple) else (body, None)
        mk = _f64(markers).reshape(-1, 3)
        a.markers_xyz = mk.ctypes.data_as(C.POINTER(C.c_double))
        a.n_markers = len(mk)
        keep.append(mk)
        if options is not None:
            opt = rig_init_bodies_options(lib, options, n_cameras, len(mk))
            a.options = C.pointer(opt)
            keep.append(opt)
    return arr, keep


def pack_rig_views(cameras, views):
    """The arrays mpe_rig_calibrate takes: cameras [(K, T_cam_rig)], views = row lists of (camera, marker xyz, pixel uv)
    -> (mpe_rig_camera array, view_begin, row_camera, row_marker_xyz, row_uv)."""
    cams = (MpeRigCamera * max(1, len(cameras)))()
    for c, (K, E) in zip(cams, cameras):
        c.K[:] = _f64(K).reshape(9)
        c.T_cam_rig[:] = _f64(E).reshape(16)
    begin = np.zeros(len(views) + 1, np.int32)
    begin[1:] = np.cumsum([len(rows) for rows in views])
    flat = [r for rows in views for r in rows]
    cam = np.ascontiguousarray([r[0] for r in flat], np.int32).reshape(-1)
    xyz = _f64([r[1] for r in flat]).reshape(-1, 3)
    uv = _f64([r[2] for r in flat]).reshape(-1, 2)
    return cams, begin, cam, xyz, uv


def rig_calibration_report_dict(rep, n_cam):
    return dict(status=rep.status, iterations=rep.iterations, views_used=rep.views_used, rows_used=rep.rows_used,
                rms_before=rep.rms_before, rms_after=rep.rms_after, last_step=rep.last_step,
                camera_state=list(rep.camera_state[:n_cam]), camera_rows=list(rep.camera_rows[:n_cam]))


def pack_body_views(cameras, views):
    """The arrays mpe_body_calibrate takes: cameras [(K, T_cam_rig)], views = row lists of (camera, marker index, pixel
    uv) -> (mpe_rig_camera array, view_begin, row_camera, row_marker, row_uv)."""
    cams = (MpeRigCamera * max(1, len(cameras)))()
    for c, (K, E) in zip(cams, cameras):
        c.K[:] = _f64(K).reshape(9)
        c.T_cam_rig[:] = _f64(E).reshape(16)
    begin = np.zeros(len(views) + 1, np.int32)
    begin[1:] = np.cumsum([len(rows) for rows in views])
    flat = [r for rows in views for r in rows]
    cam = np.ascontiguousarray([r[0] for r in flat], np.int32).reshape(-1)
    mk = np.ascontiguousarray([r[1] for r in flat], np.int32).reshape(-1)
    uv = _f64([r[2] for r in flat]).reshape(-1, 2)
    return cams, begin, cam, mk, uv


def body_calibration_report_dict(rep, n_markers):
    return dict(status=rep.status, iterations=rep.iterations, views_used=rep.views_used, rows_used=rep.rows_used,
                markers_free=rep.markers_free, scale_held=rep.scale_held,
                rms_before=rep.rms_before, rms_after=rep.rms_after, last_step=rep.last_step,
                marker_state=list(rep.marker_state[:n_markers]), marker_rows=list(rep.marker_rows[:n_markers]))


def rig_calibration_start(camera_pose, updated, reference_camera=0):
    """mpe_rig_calibration_start (host only): start values for Handle.rig_calibrate from per-camera poses.  camera_pose:
    (n_views, n_cam, 4, 4), camera <- marker frame; updated: (n_views, n_cam).  -> (T_cam_rig (n_cam, 4, 4), T_views
    (n_views, 4, 4), linked (n_cam) bool): E_ref = I, the others chained through the first view they share with a
    linked camera."""
    lib = load_library()
    P = _f64(camera_pose)
    n_views, n_cam = P.shape[0], P.shape[1]
    upd = np.ascontiguousarray(updated, np.int32).reshape(n_views, n_cam)
    E = np.zeros((n_cam, 4, 4))
    T = np.zeros((max(n_views, 1), 4, 4))
    linked = np.zeros(n_cam, np.int32)
    ip = C.POINTER(C.c_int)
    rc = lib.mpe_rig_calibration_start(_dp(P), upd.ctypes.data_as(ip), n_views, n_cam, int(reference_camera), _dp(E), _dp(T),
                                       linked.ctypes.data_as(ip))
    if rc < 0:
        raise MpeError("mpe_rig_calibration_start failed (%d)" % rc)
    return E, T[:n_views], linked.astype(bool)


class RigCalibrator:
    """Calibrates the extrinsics of a rig from the body it tracks: step() drives the lock-step entry of the trackers (one
    per camera, one handle, one marker set) as Rig.step does and keeps, for every tracker that updated, its pose and its
    rows (correspondences() over image_points() and the markers); solve() makes start values from the stored poses
    (rig_calibration_start) and runs Handle.rig_calibrate over the stored rows; rig() is a Rig with the result."""

    def __init__(self, handle, trackers, reference_camera=0):
        self.handle = handle
        self.trackers = list(trackers)
        self.reference_camera = int(reference_camera)
        self.views, self.poses, self.updated = [], [], []
        self.result = None

    def step(self, imgs, times, formats=None):
        """One time step -> (records (N), info (N, 8), updated (N)): the lock-step entry's, unchanged."""
        same = formats is None and not _is_torch(imgs[0]) and len({(np.shape(im), np.asarray(im).strides[0]) for im in imgs}) == 1
        if same:
            rec, info, upd = tracker_estimate_batch_mixed(self.trackers, imgs, times)
        else:
            rec, info, upd = tracker_estimate_batch_formats(self.trackers, imgs, times, formats)
        rows = []
        for c, t in enumerate(self.trackers):
            if not upd[c]:
                continue
            xy = t.image_points()
            rows += [(c, t.markers[m - 1].copy(), xy[j - 1].copy()) for m, j in t.correspondences()]
        self.views.append(rows)
        self.poses.append(rec["T"].reshape(len(self.trackers), 4, 4).copy())
        self.updated.append(np.asarray(upd, bool).copy())
        return rec, info, upd

    def start(self):
        """-> (T_cam_rig, T_views, linked) of rig_calibration_start over the stored poses."""
        return rig_calibration_start(np.array(self.poses), np.array(self.updated), self.reference_camera)

    def solve(self, max_iterations=50, step_tolerance=1e-10):
        """-> Handle.rig_calibrate's dict (kept as self.result), with the start values as "start"."""
        E0, T0, linked = self.start()
        cameras = [(t.K, E0[c]) for c, t in enumerate(self.trackers)]
        out = self.handle.rig_calibrate(cameras, self.views, T0, self.reference_camera, max_iterations, step_tolerance)
        out["start"] = dict(T_cam_rig=E0, T_views=T0, linked=linked)
        self.result = out
        return out

    def rig(self):
        """A Rig over the same trackers with the calibrated extrinsics."""
        if self.result is None or not self.result["ok"]:
            raise MpeError("RigCalibrator.rig: no calibration (call solve() first; it must succeed)")
        return Rig(self.handle, self.trackers, self.result["T_cam_rig"])


class BodyCalibrator:
    """Calibrates the LED positions of a body from the sequences it is tracked in: step() drives the lock-step entry of
    the trackers (one per camera, one handle, one marker set) as RigCalibrator.step does and keeps, for every tracker
    that updated, its pose and its rows as (camera, marker index, undistorted pixel) — correspondences() over
    image_points(); solve() starts from T_f = E_c^-1 P_c of the lowest camera that updated in view f and the trackers'
    markers, and runs Handle.body_calibrate over the stored rows; apply() sets the calibrated markers on every tracker.
    T_cam_rig: (N, 4, 4) extrinsics, camera <- rig; one tracker without extrinsics is the single-camera case (the
    identity)."""

    def __init__(self, handle, trackers, T_cam_rig=None):
        self.handle = handle
        self.trackers = list(trackers)
        if T_cam_rig is None:
            if len(self.trackers) != 1:
                raise MpeError("BodyCalibrator: %d trackers need their extrinsics (T_cam_rig)" % len(self.trackers))
            T_cam_rig = np.eye(4)[None]
        self.T_cam_rig = _f64(T_cam_rig).reshape(-1, 4, 4).copy()
        if len(self.T_cam_rig) != len(self.trackers):
            raise MpeError("BodyCalibrator: one extrinsic per tracker")
        self.views, self.poses, self.updated = [], [], []
        self.result = None

    def step(self, imgs, times, formats=None):
        """One time step -> (records (N), info (N, 8), updated (N)): the lock-step entry's, unchanged."""
        same = formats is None and not _is_torch(imgs[0]) and len({(np.shape(im), np.asarray(im).strides[0]) for im in imgs}) == 1
        if same:
            rec, info, upd = tracker_estimate_batch_mixed(self.trackers, imgs, times)
        else:
            rec, info, upd = tracker_estimate_batch_formats(self.trackers, imgs, times, formats)
        rows = []
        for c, t in enumerate(self.trackers):
            if not upd[c]:
                continue
            xy = t.image_points()
            rows += [(c, int(m) - 1, xy[j - 1].copy()) for m, j in t.correspondences()]
        self.views.append(rows)
        self.poses.append(rec["T"].reshape(len(self.trackers), 4, 4).copy())
        self.updated.append(np.asarray(upd, bool).copy())
        return rec, info, upd

    def start(self):
        """-> T_views (n, 4, 4): E_c^-1 P_c of the lowest camera that updated in the view, the identity if none did."""
        T = np.tile(np.eye(4), (len(self.views), 1, 1))
        for f, (P, upd) in enumerate(zip(self.poses, self.updated)):
            for c in range(len(self.trackers)):
                if upd[c]:
                    T[f] = np.linalg.inv(self.T_cam_rig[c]) @ P[c]
                    break
        return T

    def solve(self, scale=-1, max_iterations=50, step_tolerance=1e-10):
        """-> Handle.body_calibrate's dict (kept as self.result), with the start values as "start"."""
        T0 = self.start()
        markers = self.trackers[0].markers.copy()
        cameras = [(t.K, self.T_cam_rig[c]) for c, t in enumerate(self.trackers)]
        out = self.handle.body_calibrate(cameras, self.views, markers, T0, scale, max_iterations, step_tolerance)
        out["start"] = dict(markers=markers, T_views=T0)
        self.result = out
        return out

    def apply(self):
        """The calibrated markers onto every tracker (mpe_tracker_set_markers)."""
        if self.result is None or not self.result["ok"]:
            raise MpeError("BodyCalibrator.apply: no calibration (call solve() first; it must succeed)")
        for t in self.trackers:
            t.set_markers(self.result["markers"])
