"""CPU tier of the rig calibration: the steps of mpe_rig_calibrate (csrc/mpe_rig_ba.h) compiled for the host behind
mpe_rig_gn.h and the tail helpers of mpe_k3.hip, driven by the library's own row rules and iteration
(csrc/mpe_rig_ba_plan.h), and compared with a numpy witness written in another formulation (tests/witness_rig_ba.py: one
dense Jacobian over all unknowns, np.linalg.solve, no Schur complement) with the criteria the project applies to this
refinement (witness_rig.check_against_witness): extrinsics and view poses within 1e-9, covariance allclose(rtol=1e-5,
atol=1e-12), iteration counts within +-1.  Noise-free data gives the true extrinsics back; the row rules; the start helper
against a numpy restatement; the same source stand-alone (own main) plain and under AddressSanitizer +
UndefinedBehaviorSanitizer; the new declarations of include/mpe.h: valid C99, exported, ctypes sizes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rpg_monocular_pose_estimator_amd as mpe
import witness_rig
import witness_rig_ba as wba

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "rig_ba_host.cpp")
ONE_CHUNK = 1 << 40


def _extract(d):
    hip = mpe.device_source()
    i = hip.index("struct T34 {")
    with open(os.path.join(d, "k3_extract.inc"), "w") as fh:
        fh.write(hip[i:hip.index("#define K3_GROUP", i)])
    return ["-std=c++17", "-ffp-contract=off", "-I", str(d), "-I", os.path.join(ROOT, "tests", "host", "stub"), "-I", CSRC]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("rig_ba_host")
    so = os.path.join(d, "librig_ba_host.so")
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", *_extract(d), SRC, "-o", so])
    lib = C.CDLL(so)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    lib.host_rig_calibrate.argtypes = [C.c_void_p, C.c_int, ip, ip, dp, dp, C.c_int, dp, C.c_int, C.c_int, C.c_double,
                                       C.c_longlong, dp, dp, dp, ip, C.POINTER(mpe.MpeRigCalibrationReport)]
    return lib


def host_calibrate(host, prob, reference_camera=0, max_iterations=50, step_tolerance=1e-10, cap_doubles=ONE_CHUNK):
    """host_rig_calibrate -> the dict Handle.rig_calibrate returns"""
    cameras, views = prob["cameras"], prob["views"]
    cams, begin, cam, xyz, uv = mpe.binding.pack_rig_views(cameras, views)
    n, n_cam = len(views), len(cameras)
    T0 = np.ascontiguousarray(prob["T_start"], float).reshape(-1, 16)
    E, T, cov = np.zeros((n_cam, 4, 4)), np.zeros((max(n, 1), 4, 4)), np.zeros((n_cam, 6, 6))
    used = np.zeros(max(n, 1), np.int32)
    rep = mpe.MpeRigCalibrationReport()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    rc = host.host_rig_calibrate(cams, n_cam, begin.ctypes.data_as(ip), cam.ctypes.data_as(ip), xyz.ctypes.data_as(dp),
                                 uv.ctypes.data_as(dp), n, T0.ctypes.data_as(dp), reference_camera, max_iterations,
                                 step_tolerance, cap_doubles, E.ctypes.data_as(dp), T.ctypes.data_as(dp),
                                 cov.ctypes.data_as(dp), used.ctypes.data_as(ip), C.byref(rep))
    return dict(T_cam_rig=E, T_views=T[:n], cov=cov, view_used=used[:n].astype(bool),
                report=mpe.binding.rig_calibration_report_dict(rep, n_cam), ok=rc == 1)


def _same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("T_cam_rig", "T_views", "cov", "view_used")) \
        and a["report"] == b["report"]


def test_calibration_against_the_witness(host):
    """100 random problems: 2 - 8 cameras, 2 - 40 views, cameras missing from views at random, 3 - 5 of 5 markers seen,
    0.1 px noise; every fourth one again in chunks of a few views: the same bits.  The witness itself needs 5 - 8
    iterations on the problems of this seed (asserted: at most 10).  Over seven seeds of this generator 97 % of the
    problems took 5 - 7; about one in a hundred — views of 3 markers near a second solution — took the witness 9 - 14,
    and the host build stayed within +-1 of it there as well."""
    rng = np.random.default_rng(1)
    its, solved = [], 0
    for k in range(100):
        prob = wba.random_calibration(rng, int(rng.integers(2, 9)), int(rng.integers(2, 41)), p_missing=rng.uniform(0, 0.5))
        got = host_calibrate(host, prob)
        w = wba.check_against_witness(got, prob, k)
        if w["ok"]:
            its.append(w["report"]["iterations"])
            solved += 1
            assert got["report"]["rms_after"] <= got["report"]["rms_before"], k
        if k % 4 == 0:
            assert _same(host_calibrate(host, prob, cap_doubles=1000), got), k
    print("iterations of the witness: %d .. %d over %d problems" % (min(its), max(its), solved))
    assert solved >= 90 and max(its) <= 10, (solved, min(its), max(its))


def test_noise_free_data_gives_the_true_extrinsics(host):
    rng = np.random.default_rng(5)
    for k, (n_cam, n_views) in enumerate([(2, 3), (3, 12), (8, 20), (16, 6)]):
        prob = wba.random_calibration(rng, n_cam, n_views, p_missing=0.0 if n_cam == 2 else 0.2, noise=0.0)
        # (exact pixels: no rounding through float32 either)
        for f, rows in enumerate(prob["views"]):
            for i, (c, p, _) in enumerate(rows):
                K = prob["cameras"][c][0]
                q = (prob["E_true"][c] @ prob["T_true"][f] @ np.append(p, 1.0))[:3]
                rows[i] = (c, p, np.array([K[0, 0] * q[0] / q[2] + K[0, 2], K[1, 1] * q[1] / q[2] + K[1, 2]]))
        got = host_calibrate(host, prob)
        assert got["ok"] and (np.array(got["report"]["camera_state"][1:]) == 1).all(), k
        assert np.abs(got["T_cam_rig"] - prob["E_true"]).max() <= 1e-9, (k, np.abs(got["T_cam_rig"] - prob["E_true"]).max())
        used = got["view_used"]
        assert np.abs(got["T_views"][used] - prob["T_true"][used]).max() <= 1e-9, k
        wba.check_against_witness(got, prob, k)


def _rule_problem(rng):
    """4 cameras, 12 views, all cameras in all views at first"""
    return wba.random_calibration(rng, 4, 12, p_missing=0.0, seen=(4, 5))


def test_row_rules(host):
    rng = np.random.default_rng(11)
    # a view of one camera and a view of 2 rows are unused: their poses come back as given, bit for bit
    prob = _rule_problem(rng)
    prob["views"][3] = [r for r in prob["views"][3] if r[0] == 1]
    prob["views"][7] = [r for r in prob["views"][7] if r[0] in (0, 2)][:1] + [r for r in prob["views"][7] if r[0] == 2][:1]
    got = host_calibrate(host, prob)
    assert got["ok"] and list(got["view_used"]) == [f not in (3, 7) for f in range(12)]
    assert got["report"]["views_used"] == 10 and got["report"]["camera_state"] == [0, 1, 1, 1]
    for f in (3, 7):
        assert got["T_views"][f].tobytes() == np.ascontiguousarray(prob["T_start"][f]).tobytes()
    wba.check_against_witness(got, prob, "unused views")
    # a camera without rows, and a camera that only ever shares views with nobody, are held
    prob = _rule_problem(rng)
    views = []
    for rows in prob["views"]:
        views.append([r for r in rows if r[0] in (0, 1)])
        views.append([r for r in rows if r[0] == 3])
    prob["views"] = views
    prob["T_start"] = np.repeat(prob["T_start"], 2, axis=0)
    got = host_calibrate(host, prob)
    assert got["ok"] and got["report"]["camera_state"] == [0, 1, 2, 2] and got["report"]["camera_rows"][2:] == [0, 0]
    assert list(got["view_used"]) == [f % 2 == 0 for f in range(24)]
    for c in (2, 3):
        assert got["T_cam_rig"][c].tobytes() == np.ascontiguousarray(prob["cameras"][c][1]).tobytes()
        assert not got["cov"][c].any()
    assert not got["cov"][0].any() and got["cov"][1].diagonal().min() > 0
    wba.check_against_witness(got, prob, "held cameras")
    # two islands: cameras {0, 1} and {2, 3} never share a view; with reference camera 2 the other island is held
    prob = _rule_problem(rng)
    prob["views"] = [[r for r in rows if (r[0] < 2) == (f % 2 == 0)] for f, rows in enumerate(prob["views"])]
    for ref, states in ((0, [0, 1, 2, 2]), (2, [2, 2, 0, 1]), (3, [2, 2, 1, 0])):
        # (the reference camera's start value is what fixes the gauge: whatever it is, it comes back unchanged)
        got = host_calibrate(host, prob, reference_camera=ref)
        assert got["ok"] and got["report"]["camera_state"] == states, ref
        assert got["T_cam_rig"][ref].tobytes() == np.ascontiguousarray(prob["cameras"][ref][1]).tobytes()
        assert list(got["view_used"]) == [(f % 2 == 0) == (ref < 2) for f in range(12)]
        wba.check_against_witness(got, prob, ("islands", ref), reference_camera=ref)
    # the reference camera without a row: nothing to calibrate against
    prob = _rule_problem(rng)
    prob["views"] = [[r for r in rows if r[0] != 0] for rows in prob["views"]]
    got = host_calibrate(host, prob)
    assert not got["ok"] and got["report"]["status"] == 1 and got["report"]["camera_state"] == [0, 2, 2, 2]
    assert got["report"]["views_used"] == 0 and not got["view_used"].any()
    assert got["T_views"].tobytes() == np.ascontiguousarray(prob["T_start"]).tobytes()
    wba.check_against_witness(got, prob, "no reference rows")


def test_rows_of_a_view_in_any_camera_order(host):
    """The rows of every view shuffled: the same calibration within the criteria (the sums run in another order)."""
    rng = np.random.default_rng(13)
    prob = wba.random_calibration(rng, 5, 15)
    got = host_calibrate(host, prob)
    shuffled = dict(prob)
    shuffled["views"] = [[rows[i] for i in rng.permutation(len(rows))] for rows in prob["views"]]
    again = host_calibrate(host, shuffled)
    assert got["ok"] and again["ok"] and again["report"]["camera_rows"] == got["report"]["camera_rows"]
    assert np.abs(again["T_cam_rig"] - got["T_cam_rig"]).max() <= 1e-9 and np.abs(again["T_views"] - got["T_views"]).max() <= 1e-9
    wba.check_against_witness(again, shuffled, "shuffled")


def test_reference_camera_other_than_zero(host):
    rng = np.random.default_rng(17)
    for ref in (1, 4):
        prob = wba.random_calibration(rng, 5, 12, reference_camera=ref)
        got = host_calibrate(host, prob, reference_camera=ref)
        assert got["ok"] and got["report"]["camera_state"][ref] == 0
        wba.check_against_witness(got, prob, ref, reference_camera=ref)
        start = np.array([E for _, E in prob["cameras"]])
        assert np.abs(got["T_cam_rig"] - prob["E_true"]).max() < np.abs(start - prob["E_true"]).max()


def test_iteration_cap_and_tolerance(host):
    rng = np.random.default_rng(19)
    prob = wba.random_calibration(rng, 3, 10)
    got = host_calibrate(host, prob, max_iterations=2)
    assert got["report"]["iterations"] == 2 and got["report"]["last_step"] > 1e-10
    wba.check_against_witness(got, prob, "two iterations", max_iterations=2)
    loose = host_calibrate(host, prob, step_tolerance=1e-4)
    assert loose["report"]["iterations"] < host_calibrate(host, prob)["report"]["iterations"]


def _start_restatement(P, upd, ref):
    """mpe_rig_calibration_start in numpy"""
    n_views, n_cam = upd.shape
    E = np.tile(np.eye(4), (n_cam, 1, 1))
    rnd = {ref: 0}
    for k in range(1, n_cam + 1):
        grown = False
        for f in range(n_views):
            via = [c for c in range(n_cam) if upd[f, c] and c in rnd and rnd[c] < k]
            if not via:
                continue
            for c in range(n_cam):
                if upd[f, c] and c not in rnd:
                    E[c] = P[f, c] @ np.linalg.inv(P[f, via[0]]) @ E[via[0]]
                    rnd[c] = k
                    grown = True
        if not grown:
            break
    T = np.tile(np.eye(4), (n_views, 1, 1))
    for f in range(n_views):
        for c in range(n_cam):
            if upd[f, c] and c in rnd:
                T[f] = np.linalg.inv(E[c]) @ P[f, c]
                break
    return E, T, np.array([c in rnd for c in range(n_cam)])


def test_calibration_start_against_a_numpy_restatement():
    mpe.build_library()
    rng = np.random.default_rng(23)
    for k in range(30):
        n_cam, n_views, ref = int(rng.integers(1, 9)), int(rng.integers(0, 12)), 0
        ref = int(rng.integers(0, n_cam))
        E_true = np.array([E for _, E in witness_rig.random_cameras(rng, n_cam)])
        E_true = E_true @ np.linalg.inv(E_true[ref])
        T_true = np.array([witness_rig._rigid(rng, rng.uniform(0, 0.6), [0.1, -0.1, rng.uniform(1.2, 2.2)]) for _ in range(n_views)]).reshape(-1, 4, 4)
        P = np.einsum("cij,fjk->fcik", E_true, T_true).reshape(n_views, n_cam, 4, 4)
        upd = rng.random((n_views, n_cam)) < (0.3 if k % 2 else 0.8)
        P[~upd] = np.nan                                  # (a pose that did not update is not read)
        E, T, linked = mpe.rig_calibration_start(P, upd, ref)
        Ew, Tw, lw = _start_restatement(P, upd, ref)
        assert np.array_equal(linked, lw) and linked[ref], k
        assert np.abs(E - Ew).max() <= 1e-12 and (n_views == 0 or np.abs(T - Tw).max() <= 1e-12), k
        # exact poses: the linked cameras get their true extrinsics (rig frame = the reference camera)
        assert np.abs(E[linked] - E_true[linked]).max() <= 1e-12, k
        seen = upd[:, linked].any(axis=1) if n_views else np.zeros(0, bool)
        assert n_views == 0 or (np.abs(T[seen] - T_true[seen]).max() if seen.any() else 0) <= 1e-12, k
        assert n_views == 0 or (T[~seen] == np.eye(4)).all(), k
    lib = mpe.load_library()
    assert lib.mpe_rig_calibration_start(None, None, 0, 1, 0, None, None, None) == -1
    E = np.zeros(16)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    one = np.zeros(1, np.int32)
    for n_cam, ref in ((0, 0), (17, 0), (2, 2), (2, -1)):
        assert lib.mpe_rig_calibration_start(E.ctypes.data_as(dp), one.ctypes.data_as(ip), 0, n_cam, ref, E.ctypes.data_as(dp),
                                             E.ctypes.data_as(dp), None) == -1


def test_calibration_start_links_written_out_by_hand():
    """Which view links which camera, with poses that do NOT agree with one rig (so every other choice of link gives
    other numbers).  4 cameras, reference camera 1; who updated:
        view 0: 2, 3      view 1: 1, 2      view 2: 0, 2, 3      view 3: 1, 3      view 4: nobody
    Breadth first from camera 1: its neighbours first, each through the first view it shares with camera 1 — camera 2
    through view 1 and camera 3 through view 3 (not through view 0 or 2 and camera 2, although those views come
    earlier: camera 2 is no nearer to the reference camera than camera 3 is); then camera 0, through view 2 and the lowest
    camera of the level before in it, camera 2.  A view's pose comes from the lowest linked camera that updated in it."""
    mpe.build_library()
    rng = np.random.default_rng(29)
    P = np.array([[witness_rig._rigid(rng, rng.uniform(0, 0.6), rng.uniform(-0.3, 0.3, 3) + [0, 0, 1.5]) for _ in range(4)]
                  for _ in range(5)])
    upd = np.array([[0, 0, 1, 1], [0, 1, 1, 0], [1, 0, 1, 1], [0, 1, 0, 1], [0, 0, 0, 0]], bool)
    inv = np.linalg.inv
    E1 = np.eye(4)
    E2 = P[1, 2] @ inv(P[1, 1])
    E3 = P[3, 3] @ inv(P[3, 1])
    E0 = P[2, 0] @ inv(P[2, 2]) @ E2
    T = [inv(E2) @ P[0, 2], P[1, 1], inv(E0) @ P[2, 0], P[3, 1], np.eye(4)]
    E, Tv, linked = mpe.rig_calibration_start(P, upd, 1)
    assert linked.all()
    assert np.abs(E - np.array([E0, E1, E2, E3])).max() <= 1e-12
    assert np.abs(Tv - np.array(T)).max() <= 1e-12
    # (the other readings are other numbers: camera 3 through view 0 or view 2 and camera 2)
    assert np.abs(E[3] - P[0, 3] @ inv(P[0, 2]) @ E2).max() > 1e-3 and np.abs(E[3] - P[2, 3] @ inv(P[2, 2]) @ E2).max() > 1e-3
    # a camera that shares no view with a linked one stays unlinked, with the identity
    upd2 = upd.copy()
    upd2[2, 0] = False
    E, Tv, linked = mpe.rig_calibration_start(P, upd2, 1)
    assert list(linked) == [False, True, True, True] and (E[0] == np.eye(4)).all()
    assert np.abs(Tv[2] - inv(E2) @ P[2, 2]).max() <= 1e-12


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", *flags, "-DRIG_BA_HOST_MAIN", *_extract(tmp_path), SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "rig_ba_host ok:" in r.stdout, r.stdout
    return r.stdout


def test_rig_ba_on_the_host_stand_alone(tmp_path):
    out = _build_and_run(tmp_path, "rig_ba_host", ["-O2"])
    assert "up to 256 rows a view" in out and "bit for bit" in out, out


def test_rig_ba_on_the_host_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "rig_ba_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                 "-fno-omit-frame-pointer"])


C_USER = r"""
#include <stdio.h>
#include "mpe.h"
int main(void) {
  mpe_rig_calibration_options opt;
  mpe_rig_calibration_report rep;
  int (*cal)(mpe_handle*, const mpe_rig_camera*, int, const int*, const int*, const double*, const double*, int,
             const double*, const mpe_rig_calibration_options*, double*, double*, double*, int*,
             mpe_rig_calibration_report*) = mpe_rig_calibrate;
  int (*start)(const double*, const int*, int, int, int, double*, double*, int*) = mpe_rig_calibration_start;
  mpe_rig_calibration_default_options(&opt);
  printf("%d %d %d %d %g %d\n", (int)sizeof(opt), (int)sizeof(rep), opt.reference_camera, opt.max_iterations,
         opt.step_tolerance, cal && start);
  return 0;
}
"""


def test_calibration_declarations_are_c99_exported_and_sized(tmp_path):
    mpe.build_library()
    lib = mpe.load_library()
    names = {"mpe_rig_calibrate", "mpe_rig_calibration_start", "mpe_rig_calibration_default_options"}
    assert names <= set(mpe.exported_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", mpe.library_path()], text=True)
    assert names <= set(re.findall(r" T (mpe_[a-z0-9_]+)", out))
    for n in names:
        assert getattr(lib, n).argtypes is not None, n
    src = tmp_path / "rig_ba_user.c"
    src.write_text(C_USER)
    exe = str(tmp_path / "rig_ba_user")
    libdir = os.path.dirname(mpe.library_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe, "-L", libdir, "-lmpe_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert got == [str(C.sizeof(mpe.MpeRigCalibrationOptions)), str(C.sizeof(mpe.MpeRigCalibrationReport)), "0", "50", "1e-10",
                   "1"], got
    assert C.sizeof(mpe.MpeRigCalibrationOptions) == 16 and C.sizeof(mpe.MpeRigCalibrationReport) == 16 + 24 + 2 * 64
    # the refusals that need no device: a null handle is a usage error
    assert lib.mpe_rig_calibrate(None, None, 1, None, None, None, None, 0, None, None, None, None, None, None, None) == -1
