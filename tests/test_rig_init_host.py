"""CPU tier of the rig initialiser: the logic of k_rig_init_* (csrc/mpe_rig_init.h) compiled for the host behind mpe_p3p.h,
the index helpers of mpe_k2_head.h, the tail helpers of mpe_k3.hip, mpe_rig_gn.h and mpe_rig_track.h (g++,
-ffp-contract=off) and compared with a numpy witness written in another formulation (tests/witness_rig_init.py): EQUAL
reason, item count, winner, best_rows, runner_rows and match, T_hyp within 1e-9, the record with the criteria of
witness_rig_track.check_against_witness.  Problems in which the witness meets a knife edge are re-drawn; at most 1 in 10
may be.  The witness's dicts are recorded in tests/golden/rig_init_witness.json for the GPU tier; they must be this run's.  The same source runs as a stand-alone program plain and under AddressSanitizer + UndefinedBehaviorSanitizer; the
new declarations of include/mpe.h are checked (valid C99, exported, ctypes sizes, the refusals that need no device); and
the seed of the GPU tier's scenario is checked here on the oracle's detections."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rpg_monocular_pose_estimator_amd as mpe
import witness_rig_init as WI
import witness_rig_track as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "rig_init_host.cpp")


def extract(d):
    """the cut-outs of the kernel text the host build stands on -> the g++ flags"""
    hip = mpe.device_source()
    i = hip.index("struct T34 {")
    with open(os.path.join(d, "k3_extract.inc"), "w") as fh:
        fh.write(hip[i:hip.index("#define K3_GROUP", i)])
    i = hip.index("__device__ __forceinline__ void unrank_combo3")
    with open(os.path.join(d, "k2_head_extract.inc"), "w") as fh:
        fh.write(hip[i:hip.index("}\n", hip.index("double pick_root", i)) + 2])
    return ["-std=c++17", "-ffp-contract=off", "-I", str(d), "-I", os.path.join(ROOT, "tests", "host", "stub"), "-I", CSRC]


def build_host(d):
    so = os.path.join(d, "librig_init_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", *extract(d), SRC, "-o", so])
    lib = C.CDLL(so)
    lib.host_rig_init.restype = None
    lib.host_rig_init_chunked.restype = None
    lib.host_rig_init_lds_bytes.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("rig_init_host"))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_init(host, problem, chunk=0, **options):
    """-> (record, match (n_cam, n_mk), info) of one problem through the host build"""
    cameras, markers, dets, tol_v, tol_a = problem
    o = dict(WI.DEFAULTS, **options)
    cams = mpe.binding.pack_rig_cameras(cameras)
    mk = np.ascontiguousarray(markers, float).reshape(-1, 3)
    lists = [np.ascontiguousarray(d, float).reshape(-1, 2) for d in dets]
    begin = np.zeros(len(lists) + 1, np.int32)
    begin[1:] = np.cumsum([len(d) for d in lists])
    xy = np.ascontiguousarray(np.concatenate(lists), float)
    tv, ta = np.ascontiguousarray(tol_v, float), np.ascontiguousarray(tol_a, float)
    rec = np.zeros(1, mpe.RESULT_DTYPE)
    match = np.full((len(cameras), len(mk)), 0xFFFFFFFF, np.uint32)
    info = np.zeros(1, mpe.RIG_INIT_INFO_DTYPE)
    host.host_rig_init_chunked(cams, len(cameras), _ptr(mk), len(mk), _ptr(begin), _ptr(xy), _ptr(tv), _ptr(ta), o["max_rounds"],
                               o["min_rows"], o["min_markers"], o["min_margin"], int(chunk), _ptr(rec), _ptr(match), _ptr(info))
    return rec[0], match, info[0]


@pytest.fixture(scope="module")
def drawn():
    return WI.drawn_problems()


def test_drawn_problems_against_the_witness(host, drawn):
    problems, redraws = drawn
    assert len(problems) == 80 and redraws <= len(problems) // 10, redraws
    reasons, by_kind = {}, {}
    for k, p in enumerate(problems):
        rec, match, info = host_init(host, p["problem"])
        WI.check_against_witness(rec, match, info, p["problem"], None, k, w=p["w"])
        reasons[p["w"]["reason"]] = reasons.get(p["w"]["reason"], 0) + 1
        by_kind.setdefault(str(p["kind"]), []).append(p["w"]["reason"])
        if p["kind"] is None:
            assert p["w"]["status"] != 0, k                  # no body, no pose
        elif p["w"]["status"] == 0:                          # a pose that is given is the body's
            assert np.abs(p["w"]["T"] - p["T_true"])[:3, 3].max() < 5e-3, (k, p["kind"])
    # the record the GPU tier reads instead of running the witness again is this run's
    record = WI.recorded()["drawn"]
    assert len(record) == len(problems)
    for k, p in enumerate(problems):
        assert record[k]["attempt"] == p["attempt"] and WI.same_witness(WI.unpack(record[k]), p["w"]), k
    print("re-drawn: %d of %d; reasons: %s" % (redraws, len(problems), sorted(reasons.items())))
    for kind, rs in by_kind.items():
        print("  %-12s %s" % (kind, {r: rs.count(r) for r in sorted(set(rs))}))
    assert {0, 1, 5} <= set(reasons), reasons


def test_the_exact_shapes(host):
    shapes, redraws = WI.shapes()
    assert redraws <= 1, redraws
    for s in shapes:
        rec, match, info = host_init(host, s["problem"], **s["options"])
        WI.check_against_witness(rec, match, info, s["problem"], s["options"], s["name"], w=s["w"])
        WI.check_expectation(s, s["w"])
    record = WI.recorded()["shapes"]
    assert len(record) == len(shapes)
    for r, s in zip(record, shapes):
        assert r["attempt"] == s["attempt"] and WI.same_witness(WI.unpack(r), s["w"]), s["name"]
    assert [s["name"] for s in shapes] == ["one_camera_three", "collinear", "tie", "tie_no_margin", "behind", "three_markers",
                                          "three_markers_allowed", "sixteen_by_two"]


def test_a_list_of_64_detections(host):
    problem, expect = WI.long_list()
    rec, match, info = host_init(host, problem)
    WI.check_long_list(rec, match, info, expect)


def test_the_chunk_does_not_show(host, drawn):
    for k, p in enumerate(drawn[0][:12]):
        a = host_init(host, p["problem"])
        for chunk in (1, 37, 4096):
            b = host_init(host, p["problem"], chunk=chunk)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (k, chunk)


def test_lds_leaves_four_blocks_on_a_compute_unit(host):
    assert 4 * host.host_rig_init_lds_bytes() <= 160 * 1024


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", *flags, "-DRIG_INIT_HOST_MAIN", *extract(tmp_path), SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "rig_init_host ok:" in r.stdout, r.stdout
    return r.stdout


def test_rig_init_on_the_host_stand_alone(tmp_path):
    out = _build_and_run(tmp_path, "rig_init_host", ["-O2"])
    assert "336 items decoded" in out and "12 rigs" in out, out


def test_rig_init_on_the_host_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "rig_init_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                   "-fno-omit-frame-pointer"])


C_USER = r"""
#include <stdio.h>
#include "mpe.h"
int main(void) {
  mpe_rig_init_options opt;
  mpe_rig_init_info info;
  int (*batch)(mpe_handle*, const mpe_rig_camera*, int, const double*, int, const int*, const double*, const double*,
               const double*, int, const mpe_rig_init_options*, mpe_result*, uint32_t*, mpe_rig_init_info*) = mpe_rig_init_batch;
  int (*trackers)(mpe_tracker* const*, int, const double*, const mpe_rig_init_options*, mpe_result*, uint32_t*,
                  mpe_rig_init_info*) = mpe_rig_init_trackers;
  mpe_rig_init_default_options(&opt);
  info.reason = 0;
  printf("%d %d %d %d %d %d %d\n", (int)sizeof(opt), (int)sizeof(info), opt.max_rounds, opt.min_rows, opt.min_markers,
         opt.min_margin, (batch && trackers) + info.reason);
  return 0;
}
"""


def test_rig_init_declarations_are_c99_exported_and_sized(tmp_path):
    mpe.build_library()
    lib = mpe.load_library()
    names = {"mpe_rig_init_batch", "mpe_rig_init_trackers", "mpe_rig_init_default_options"}
    assert names <= set(mpe.exported_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", mpe.library_path()], text=True)
    assert names <= set(re.findall(r" T (mpe_[a-z0-9_]+)", out))
    src = tmp_path / "rig_init_user.c"
    src.write_text(C_USER)
    exe = str(tmp_path / "rig_init_user")
    libdir = os.path.dirname(mpe.library_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe, "-L", libdir, "-lmpe_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert got == [str(C.sizeof(mpe.MpeRigInitOptions)), str(C.sizeof(mpe.MpeRigInitInfo)), "2", "6", "4", "1", "1"], got
    assert C.sizeof(mpe.MpeRigInitOptions) == 16 and C.sizeof(mpe.MpeRigInitInfo) == 224
    assert mpe.RIG_INIT_INFO_DTYPE.itemsize == 224 and mpe.RIG_INIT_INFO_DTYPE.fields["track"][1] == 192
    assert lib.mpe_rig_init_batch(None, None, 1, None, 1, None, None, None, None, 0, None, None, None, None) == -1
    assert lib.mpe_rig_init_trackers(None, 0, None, None, None, None, None) == -1
    lib.mpe_rig_init_default_options(None)               # (ignored)
    assert "mpe_rig_init.h" in open(os.path.join(CSRC, "Makefile")).read()
    assert '#include "mpe_rig_init.h"' in mpe.device_source()


# ---- the scenario of the GPU tier (tests/test_rig_init.py): the body partly hidden from EVERY camera from frame 0 on ----

def test_the_scenario_seed_on_the_oracles_detections(host, orc, tmp_path):
    """The end-to-end scenario of tests/test_rig_init.py on the CPU: the oracle's whole-image detections (findLeds) of
    every camera; frame 0 through the host build of the initialiser (back-projection tolerance for the vote and the accept
    test, as mpe_rig_init_trackers), the later frames through the host build of the tracking step from the predicted rig
    pose as Rig.step(partial=True) does.  The translation on every frame must be within HALF the bound the GPU tier
    applies (5e-3 m)."""
    import test_rig_track_host as TH
    seq, cams, E = WI.scenario_sequence()
    S = WI.SCENARIO
    P = mpe.demo_params()
    params = orc.make_params()
    cameras = [(K, E[c]) for c, (K, _, _, _) in enumerate(seq["cameras"])]
    tol_b = np.full(3, P.back_projection_pixel_tolerance)
    tol_m = np.full(3, P.nearest_neighbour_pixel_tolerance)
    so = str(tmp_path / "librig_track_host.so")            # (the tracking step's host build, for the frames behind frame 0)
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", *TH._extract(tmp_path), TH.SRC, "-o", so])
    track_host = C.CDLL(so)
    track_host.host_rig_track.restype = None
    poses, worst = [], 0.0
    for k in range(S["frames"]):
        dets = [orc.find_leds(seq["frames"][c][k], params, K, D)[0] for c, (K, D, _, _) in enumerate(seq["cameras"])]
        assert [len(x) for x in dets] == [3, 3, 2], k
        if k == 0:
            rec, match, info = host_init(host, (cameras, seq["markers"], dets, tol_b, tol_b))
            assert info["reason"] == 0 and info["best_rows"] == 8 and info["track"]["rows"] == 8, info
        else:
            t = seq["times"]
            T_pred = poses[-1] if len(poses) < 2 else mpe.predict_pose(poses[-1], poses[-2], t[k - 1], t[k - 2], t[k])
            rec, match, info = TH.host_track(track_host, (cameras, seq["markers"], dets, T_pred, tol_m, tol_b))
            assert info["reason"] == 0 and info["rows"] == 8, (k, info)
        assert rec["status"] == 0 and rec["n_det"] == 3
        for c, ms in S["partial"].items():
            assert [m for m in range(5) if match[c, m]] == list(ms), (k, c, match[c])
        err = np.abs(rec["T"].reshape(4, 4) - seq["T_true"][k])[:3, 3].max()
        worst = max(worst, err)
        poses.append(rec["T"].reshape(4, 4).copy())
    print("largest translation error: %.3g m" % worst)
    assert worst <= 2.5e-3, worst

