"""CPU tier of the rig's partial-view tracking step: the logic of k_rig_track (csrc/mpe_rig_track.h) compiled for the host
behind mpe_rig_gn.h and the tail helpers of mpe_k3.hip (g++, -ffp-contract=off) and compared with a numpy witness written
in another formulation (tests/witness_rig_track.py: dense distance matrices with argmin, uniqueness by sorting,
witness_rig.rig_optimise_pose for the refinement) with the criteria the project applies to this refinement (pose within
1e-9, covariance allclose(rtol=1e-5, atol=1e-12), iterations +-1) and EQUAL match, rounds and reason.  Problems in which a
comparison falls within 1e-6 px of its tolerance are re-drawn (the witness measures it); at most 5 % may be.  Pins: one
round is rig_gn_refine over the matched rows bit for bit, two rounds are two chained single rounds.  The same source runs
as a stand-alone program plain and under AddressSanitizer + UndefinedBehaviorSanitizer; the new declarations of
include/mpe.h are checked (valid C99, exported, ctypes sizes, the refusals that need no device); synth.make_rig_sequence
keeps its bytes; and the seed of the GPU tier's scenario is checked here on the oracle's detections."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import rpg_monocular_pose_estimator_amd as mpe
from rpg_monocular_pose_estimator_amd import synth
import witness_rig_track as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "rig_track_host.cpp")
INF = float("inf")


def _extract(d):
    hip = mpe.device_source()
    i = hip.index("struct T34 {")
    with open(os.path.join(d, "k3_extract.inc"), "w") as fh:
        fh.write(hip[i:hip.index("#define K3_GROUP", i)])
    return ["-std=c++17", "-ffp-contract=off", "-I", str(d), "-I", os.path.join(ROOT, "tests", "host", "stub"), "-I", CSRC]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("rig_track_host")
    so = os.path.join(d, "librig_track_host.so")
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", *_extract(d), SRC, "-o", so])
    lib = C.CDLL(so)
    lib.host_rig_track.restype = None
    lib.host_rig_refine.restype = None
    lib.host_rig_track_lds_bytes.restype = C.c_int
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_track(host, problem, max_rounds=2, min_rows=4, min_markers=3):
    """-> (record, match (n_cam, n_mk), info) of one problem through the host build"""
    cameras, markers, dets, T_pred, tol_m, tol_a = problem
    cams = mpe.binding.pack_rig_cameras(cameras)
    mk = np.ascontiguousarray(markers, float).reshape(-1, 3)
    lists = [np.ascontiguousarray(d, float).reshape(-1, 2) for d in dets]
    begin = np.zeros(len(lists) + 1, np.int32)
    begin[1:] = np.cumsum([len(d) for d in lists])
    xy = np.ascontiguousarray(np.concatenate(lists), float)
    T0 = np.ascontiguousarray(T_pred, float)
    tm, ta = np.ascontiguousarray(tol_m, float), np.ascontiguousarray(tol_a, float)
    rec = np.zeros(1, mpe.RESULT_DTYPE)
    match = np.full((len(cameras), len(mk)), 0xFFFFFFFF, np.uint32)
    info = np.zeros(1, mpe.RIG_TRACK_INFO_DTYPE)
    host.host_rig_track(cams, len(cameras), _ptr(mk), len(mk), _ptr(begin), _ptr(xy), _ptr(tm), _ptr(ta), _ptr(T0),
                        max_rounds, min_rows, min_markers, _ptr(rec), _ptr(match), _ptr(info))
    return rec[0], match, info[0]


def host_refine(host, cameras, rows, T0):
    cams = mpe.binding.pack_rig_cameras(cameras)
    cam = np.ascontiguousarray([r[0] for r in rows], np.int32)
    xyz = np.ascontiguousarray([r[1] for r in rows], float).reshape(-1, 3)
    uv = np.ascontiguousarray([r[2] for r in rows], float).reshape(-1, 2)
    T0 = np.ascontiguousarray(T0, float)
    rec = np.zeros(1, mpe.RESULT_DTYPE)
    host.host_rig_refine(cams, len(cameras), _ptr(cam), _ptr(xyz), _ptr(uv), len(rows), _ptr(T0), _ptr(rec))
    return rec[0]


def random_problems(seed, n):
    """n drawn problems of mixed kinds (plain, a displaced detection, a far start, many detections, few LEDs) -> (list of (problem,
    options, witness dict), re-draws)"""
    rng = np.random.default_rng(seed)
    out, redraws = [], 0
    for k in range(n):
        kw, options = {}, {}
        if k % 4 == 1:
            kw = dict(n_cam=3, seen=[4, 3, 3], displace=(int(rng.integers(0, 3)), float(rng.uniform(4, 11))))
        elif k % 4 == 2:
            kw = dict(start=(0.008, 0.01), clutter=int(rng.integers(0, 30)))
        elif k % 8 == 3:
            kw = dict(n_cam=2, seen=[int(rng.integers(0, 4)), int(rng.integers(0, 3))], clutter=1)
        if k % 3 == 0:
            options = dict(max_rounds=int(rng.integers(1, 5)))
        problem, _, w, r = W.draw(rng, options, **kw)
        redraws += r
        out.append((problem, options, w))
    return out, redraws


def test_tracking_step_against_the_witness(host):
    problems, redraws = random_problems(2024, 300)
    assert redraws <= 0.05 * len(problems), redraws
    seen = {}
    for k, (problem, options, w) in enumerate(problems):
        rec, match, info = host_track(host, problem, **options)
        W.check_against_witness(rec, match, info, problem, options, k)
        seen[(w["reason"], w["rounds"])] = seen.get((w["reason"], w["rounds"]), 0) + 1
    print("re-drawn: %d of %d; (reason, rounds): %s" % (redraws, len(problems), sorted(seen.items())))
    # the draw reaches a pose in one and in two rounds, a rejected pose and a row set that is too small
    assert {(0, 1), (0, 2), (4, 1)} <= set(seen) and any(r == 1 for r, _ in seen), seen


def test_the_smallest_shapes_that_can_go_wrong(host):
    shapes, redraws = W.shapes()
    assert redraws <= 1, redraws                         # (5 % of the drawn shapes is less than one)
    for s in shapes:
        rec, match, info = host_track(host, s["problem"], **s["options"])
        w = W.check_against_witness(rec, match, info, s["problem"], s["options"], s["name"])
        W.check_expectation(s, w)
    names = [s["name"] for s in shapes]
    assert {"1x4", "16x16", "behind", "three_rows", "two_markers", "outlier_1", "outlier_2", "claimed_distinct",
            "claimed_tie", "detection_tie"} <= set(names)
    big = shapes[names.index("16x16")]["problem"]
    assert len(big[0]) * len(big[1]) == 256 and sorted(len(d) for d in big[2])[::len(big[2]) - 1] == [0, 64]


def test_one_round_is_the_refinement_over_the_matched_rows_bit_for_bit(host):
    problems, _ = random_problems(11, 60)
    shapes, _ = W.shapes()
    n = 0
    for problem, _, _ in problems + [(s["problem"], None, None) for s in shapes]:
        rec, match, info = host_track(host, problem, max_rounds=1)
        if rec["status"] != 0:
            continue
        rows = W.rows_of(match.astype(np.int64), problem[1], problem[2])
        ref = host_refine(host, problem[0], rows, problem[3])
        assert ref.tobytes() == rec.tobytes(), (n, info)
        n += 1
    assert n >= 40, n


def chained(track, problem):
    """two single rounds in a row, as the two-round call runs them -> (record, match, info) it must return"""
    cameras, markers, dets, T_pred, tol_m, tol_a = problem
    inf = np.full(len(cameras), INF)
    r1, m1, i1 = track((cameras, markers, dets, T_pred, tol_m, inf), max_rounds=1)
    if r1["status"] != 0:                                # reasons 1 .. 3 of round 0
        return r1, m1, i1
    r2, m2, i2 = track((cameras, markers, dets, r1["T"].reshape(4, 4), tol_a, tol_a), max_rounds=1)
    if np.array_equal(m1, m2):                           # a stable row set: the first refinement, accepted or not by tol_a
        return track((cameras, markers, dets, T_pred, tol_m, tol_a), max_rounds=1)
    return r2, m2, i2


def test_two_rounds_are_two_chained_single_rounds(host):
    problems, _ = random_problems(12, 80)
    shapes, _ = W.shapes()
    kinds = set()
    for k, (problem, _, _) in enumerate(problems + [(s["problem"], None, None) for s in shapes]):
        rec, match, info = host_track(host, problem, max_rounds=2)
        r, m, i = chained(lambda p, **o: host_track(host, p, **o), problem)
        assert np.array_equal(match, m) and info["reason"] == i["reason"] and info["rows"] == i["rows"], k
        assert rec["status"] == r["status"] and rec["gn_iterations"] == r["gn_iterations"], k
        if rec["status"] == 0:
            assert rec["T"].tobytes() == r["T"].tobytes() and rec["cov"].tobytes() == r["cov"].tobytes(), k
        else:                                            # without a pose the two-round call hands back ITS start
            assert np.array_equal(rec["T"].reshape(4, 4), np.asarray(problem[3], float)) and not rec["cov"].any(), k
        kinds.add((int(info["reason"]), int(info["rounds"])))
    assert {(0, 1), (0, 2)} <= kinds, kinds


def test_lds_leaves_three_blocks_on_a_compute_unit(host):
    assert 3 * host.host_rig_track_lds_bytes() <= 160 * 1024 and host.host_rig_track_lds_bytes() < 64 * 1024


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", *flags, "-DRIG_TRACK_HOST_MAIN", *_extract(tmp_path), SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "rig_track_host ok:" in r.stdout, r.stdout
    return r.stdout


def test_rig_track_on_the_host_stand_alone(tmp_path):
    out = _build_and_run(tmp_path, "rig_track_host", ["-O2"])
    assert "80 rigs" in out and "160 records bit-equal" in out and "3 without a pose" in out, out


def test_rig_track_on_the_host_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "rig_track_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                    "-fno-omit-frame-pointer"])


C_USER = r"""
#include <stdio.h>
#include "mpe.h"
int main(void) {
  mpe_rig_track_options opt;
  mpe_rig_track_info info;
  int (*batch)(mpe_handle*, const mpe_rig_camera*, int, const double*, int, const int*, const double*, const double*,
               const double*, int, const double*, const mpe_rig_track_options*, mpe_result*, uint32_t*,
               mpe_rig_track_info*) = mpe_rig_track_batch;
  int (*trackers)(mpe_tracker* const*, int, const double*, const double[16], const mpe_rig_track_options*, mpe_result*,
                  uint32_t*, mpe_rig_track_info*) = mpe_rig_track_trackers;
  mpe_rig_track_default_options(&opt);
  info.reason = 0;
  printf("%d %d %d %d %d %d\n", (int)sizeof(opt), (int)sizeof(info), opt.max_rounds, opt.min_rows, opt.min_markers,
         (batch && trackers) + info.reason);
  return 0;
}
"""


def test_rig_track_declarations_are_c99_exported_and_sized(tmp_path):
    mpe.build_library()
    lib = mpe.load_library()
    names = {"mpe_rig_track_batch", "mpe_rig_track_trackers", "mpe_rig_track_default_options"}
    assert names <= set(mpe.exported_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", mpe.library_path()], text=True)
    assert names <= set(re.findall(r" T (mpe_[a-z0-9_]+)", out))
    for n in names:
        assert getattr(lib, n).argtypes is not None, n
    src = tmp_path / "rig_track_user.c"
    src.write_text(C_USER)
    exe = str(tmp_path / "rig_track_user")
    libdir = os.path.dirname(mpe.library_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe, "-L", libdir, "-lmpe_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert got == [str(C.sizeof(mpe.MpeRigTrackOptions)), str(C.sizeof(mpe.MpeRigTrackInfo)), "2", "4", "3", "1"], got
    assert C.sizeof(mpe.MpeRigTrackOptions) == 12 and C.sizeof(mpe.MpeRigTrackInfo) == 32
    assert mpe.RIG_TRACK_INFO_DTYPE.itemsize == 32
    # the refusals that need no device: a null handle or pointer is a usage error
    assert lib.mpe_rig_track_batch(None, None, 1, None, 1, None, None, None, None, 0, None, None, None, None, None) == -1
    assert lib.mpe_rig_track_trackers(None, 0, None, None, None, None, None, None) == -1
    lib.mpe_rig_track_default_options(None)              # (ignored)
    assert mpe.source_fingerprint() and "mpe_rig_track.h" in open(os.path.join(CSRC, "Makefile")).read()
    assert "rig_track(" in mpe.device_source() or '#include "mpe_rig_track.h"' in mpe.device_source()


def _sequence_digest(seq):
    m = hashlib.sha256()
    for f in seq["frames"]:
        m.update(np.ascontiguousarray(f).tobytes())
    m.update(seq["T_true"].tobytes())
    return m.hexdigest()


def test_make_rig_sequence_keeps_its_bytes_and_renders_the_stated_leds():
    cams, E = W.rig_cameras(2)
    # (the digest of this call before `visible` existed)
    before = "9d5f3d347ef3577726b35233436ce688b4ddf320804533a4d0e83d9ef2ed9f9e"
    plain = synth.make_rig_sequence("C2", 6, 5, cams, E, dropout={1: (3,)})
    assert _sequence_digest(plain) == before
    assert _sequence_digest(synth.make_rig_sequence("C2", 6, 5, cams, E, dropout={1: (3,)}, visible=None)) == before
    vis = {0: {2: (0, 3)}, 1: {3: (1, 2, 4), 4: ()}}
    seq = synth.make_rig_sequence("C2", 6, 5, cams, E, dropout={1: (3,)}, visible=vis)
    assert np.array_equal(seq["T_true"], plain["T_true"])
    for c, (K, D, rows, cols) in enumerate(seq["cameras"]):
        px = [synth.distort_px(synth.project(E[c] @ T, seq["markers"], K), K, D) for T in seq["T_true"]]
        for k in range(6):
            lit = [bool(seq["frames"][c][k][int(round(y)), int(round(x))] > 200) for x, y in px[k]]
            want = [m in vis[c][k] for m in range(5)] if k in vis.get(c, ()) else [True] * 5
            assert lit == want, (c, k, lit)
            if k not in vis.get(c, ()):
                assert np.array_equal(seq["frames"][c][k], plain["frames"][c][k]), (c, k)
            # nothing bright but the stated LEDs: every bright pixel lies within 8 px of one of them
            ys, xs = np.nonzero(seq["frames"][c][k] > 120)
            shown = np.array([px[k][m] for m in range(5) if want[m]]).reshape(-1, 2)
            assert len(ys) == 0 or (len(shown) and (np.hypot(xs[:, None] - shown[None, :, 0], ys[:, None] - shown[None, :, 1])
                                                    .min(axis=1) < 8).all()), (c, k)


def test_the_scenario_seed_on_the_oracles_detections(host, orc):
    """The scenario of tests/test_rig_tracking.py on the CPU: the oracle's whole-image detections (findLeds) of every
    camera through the host build of the tracking step, the rig pose predicted from the last two as Rig.step(partial=True)
    does.  The translation on every partial frame must be within HALF the bound the GPU tier applies (5e-3 m).  Observed
    with seed 6: 1.40 mm at the most (seeds 1 .. 12 scanned: 1.4 mm to 9.3 mm, the depth of a body 1.3 .. 2.4 m away)."""
    seq, cams, E = W.scenario_sequence()
    S = W.SCENARIO
    P = mpe.demo_params()
    params = orc.make_params()
    tol_m = np.full(3, P.nearest_neighbour_pixel_tolerance)
    tol_a = np.full(3, P.back_projection_pixel_tolerance)
    cameras = [(K, E[c]) for c, (K, _, _, _) in enumerate(seq["cameras"])]
    poses, worst = [seq["T_true"][0]], 0.0               # (frame 0: the fused pose stands within a millimetre of the truth)
    for k in range(1, S["frames"]):
        t = seq["times"]
        T_pred = poses[-1] if len(poses) < 2 else mpe.predict_pose(poses[-1], poses[-2], t[k - 1], t[k - 2], t[k])
        dets = [orc.find_leds(seq["frames"][c][k], params, K, D)[0] for c, (K, D, _, _) in enumerate(seq["cameras"])]
        partial = k >= S["full"]
        assert [len(d) for d in dets] == ([len(S["partial"][c]) for c in range(3)] if partial else [5, 5, 5]), k
        rec, match, info = host_track(host, (cameras, seq["markers"], dets, T_pred, tol_m, tol_a))
        assert rec["status"] == 0 and info["reason"] == 0 and info["rows"] == (8 if partial else 15), (k, info)
        err = np.abs(rec["T"].reshape(4, 4) - seq["T_true"][k])[:3, 3].max()
        if partial:
            assert rec["n_det"] == 3
            for c, ms in S["partial"].items():
                assert [m for m in range(5) if match[c, m]] == list(ms), (k, c, match[c])
            worst = max(worst, err)
        poses.append(rec["T"].reshape(4, 4).copy())
    print("largest translation error on a partial frame: %.3g m" % worst)
    assert worst <= 2.5e-3, worst
