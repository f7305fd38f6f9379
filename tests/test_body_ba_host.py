"""CPU tier of the marker calibration: the steps of mpe_body_calibrate (csrc/mpe_body_ba.h) compiled for the host behind
mpe_rig_gn.h, mpe_rig_ba.h and the tail helpers of mpe_k3.hip, driven by the library's own row rules
(csrc/mpe_body_ba_plan.h) and iteration (csrc/mpe_rig_ba_plan.h), and compared with a numpy witness written in another
formulation (tests/witness_body_ba.py: one dense Jacobian over all unknowns, the inner constraints as the border of a KKT
system, np.linalg.solve, the covariance from np.linalg.pinv) with witness_rig_ba's criteria: marker positions and view
poses within 1e-9, covariance allclose(rtol=1e-5, atol=1e-12), iteration counts within +-1.  Noise-free data gives the
true shape back; every row rule; the scale option; the constraints; the same source stand-alone (own main) plain and
under AddressSanitizer + UndefinedBehaviorSanitizer; the new declarations of include/mpe.h: valid C99, exported, ctypes
sizes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rpg_monocular_pose_estimator_amd as mpe
import witness_body_ba as wbb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "body_ba_host.cpp")
ONE_CHUNK = 1 << 40


def _extract(d):
    hip = mpe.device_source()
    i = hip.index("struct T34 {")
    with open(os.path.join(d, "k3_extract.inc"), "w") as fh:
        fh.write(hip[i:hip.index("#define K3_GROUP", i)])
    return ["-std=c++17", "-ffp-contract=off", "-I", str(d), "-I", os.path.join(ROOT, "tests", "host", "stub"), "-I", CSRC]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("body_ba_host")
    so = os.path.join(d, "libbody_ba_host.so")
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", *_extract(d), SRC, "-o", so])
    lib = C.CDLL(so)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    lib.host_body_calibrate.argtypes = [C.c_void_p, C.c_int, dp, C.c_int, ip, ip, ip, dp, C.c_int, dp, C.c_int, C.c_int,
                                        C.c_double, C.c_longlong, dp, dp, dp, ip, C.POINTER(mpe.MpeBodyCalibrationReport)]
    return lib


def host_calibrate(host, prob, scale=-1, max_iterations=50, step_tolerance=1e-10, cap_doubles=ONE_CHUNK):
    """host_body_calibrate -> the dict Handle.body_calibrate returns"""
    cameras, views = prob["cameras"], prob["views"]
    cams, begin, cam, mk_idx, uv = mpe.pack_body_views(cameras, views)
    n, n_cam = len(views), len(cameras)
    mk = np.ascontiguousarray(prob["markers"], float).reshape(-1, 3)
    T0 = np.ascontiguousarray(prob["T_start"], float).reshape(-1, 16)
    P, T, cov = np.zeros((len(mk), 3)), np.zeros((max(n, 1), 4, 4)), np.zeros((len(mk), 3, 3))
    used = np.zeros(max(n, 1), np.int32)
    rep = mpe.MpeBodyCalibrationReport()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    rc = host.host_body_calibrate(cams, n_cam, mk.ctypes.data_as(dp), len(mk), begin.ctypes.data_as(ip), cam.ctypes.data_as(ip),
                                  mk_idx.ctypes.data_as(ip), uv.ctypes.data_as(dp), n, T0.ctypes.data_as(dp), scale,
                                  max_iterations, step_tolerance, cap_doubles, P.ctypes.data_as(dp), T.ctypes.data_as(dp),
                                  cov.ctypes.data_as(dp), used.ctypes.data_as(ip), C.byref(rep))
    return dict(markers=P, T_views=T[:n], cov=cov, view_used=used[:n].astype(bool),
                report=mpe.binding.body_calibration_report_dict(rep, len(mk)), ok=rc == 1)


def _same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("markers", "T_views", "cov", "view_used")) \
        and a["report"] == b["report"]


def test_calibration_against_the_witness(host):
    """100 random problems: 1 - 8 cameras, 4 - 40 views, 4 - 8 markers, every row missing with a probability drawn from
    0 .. 0.3, 0.1 px noise, start markers 4 mm off; every fourth one again in chunks of a few views: the same bits.  The
    witness itself needs 5 - 7 iterations on the problems of this seed (asserted: at most 10) and solves all of them
    (asserted: at least 90).  Over seven seeds of this generator (700 problems) six — four markers, or views of four
    rows — took the witness 11 - 17 (plain Gauss-Newton on a non-zero residual converges linearly there), and two (2
    cameras with 4 markers) ran to the iteration cap or one short of it."""
    rng = np.random.default_rng(2)
    its, solved = [], 0
    for k in range(100):
        prob = wbb.random_body_calibration(rng, int(rng.integers(1, 9)), int(rng.integers(4, 41)), int(rng.integers(4, 9)),
                                           p_missing=rng.uniform(0, 0.3))
        got = host_calibrate(host, prob)
        w = wbb.check_against_witness(got, prob, k)
        if w["ok"]:
            its.append(w["report"]["iterations"])
            solved += 1
            assert got["report"]["rms_after"] <= got["report"]["rms_before"], k
        if k % 4 == 0:
            assert _same(host_calibrate(host, prob, cap_doubles=1000), got), k
    print("iterations of the witness: %d .. %d over %d problems" % (min(its), max(its), solved))
    assert solved >= 90 and max(its) <= 10, (solved, min(its), max(its))


def test_noise_free_data_gives_the_true_shape(host):
    """Exact pixels: after a rigid alignment (a similarity when scale is held) the true shape is back within 1e-9."""
    rng = np.random.default_rng(5)
    for k, (n_cam, n_views, n_mk) in enumerate([(1, 12, 5), (1, 6, 4), (2, 4, 4), (3, 8, 5), (8, 20, 8), (16, 6, 16)]):
        prob = wbb.random_body_calibration(rng, n_cam, n_views, n_mk, p_missing=0.0 if n_views < 8 else 0.2, exact=True)
        got = host_calibrate(host, prob)
        assert got["ok"] and got["report"]["marker_state"] == [1] * n_mk, k
        assert got["report"]["scale_held"] == (1 if n_cam == 1 else 0), k
        err = wbb.shape_error(got["markers"], prob["markers_true"], with_scale=n_cam == 1)
        assert err <= 1e-9, (k, err)
        assert got["report"]["rms_after"] <= 1e-9, k
        wbb.check_against_witness(got, prob, k)


def _rule_problem(rng, n_cam=2, n_mk=6):
    """12 views, every camera sees every marker in every view"""
    return wbb.random_body_calibration(rng, n_cam, 12, n_mk, p_missing=0.0)


def test_row_rules(host):
    rng = np.random.default_rng(11)
    # a view of 3 rows, and a view of 4 rows on 2 markers, are unused: their poses come back as given, bit for bit
    prob = _rule_problem(rng)
    prob["views"][3] = prob["views"][3][:3]
    prob["views"][7] = [r for r in prob["views"][7] if r[1] in (0, 1)]
    got = host_calibrate(host, prob)
    assert got["ok"] and list(got["view_used"]) == [f not in (3, 7) for f in range(12)]
    assert got["report"]["views_used"] == 10 and got["report"]["marker_state"] == [1] * 6
    for f in (3, 7):
        assert got["T_views"][f].tobytes() == np.ascontiguousarray(prob["T_start"][f]).tobytes()
    wbb.check_against_witness(got, prob, "unused views")
    # a marker with one row, and a marker without a row, are held: positions as given bit for bit, zero covariance
    prob = _rule_problem(rng)
    seen = [False]
    def keep(r):
        if r[1] == 4:
            return False
        if r[1] == 5:
            first, seen[0] = not seen[0], True
            return first
        return True
    prob["views"] = [[r for r in rows if keep(r)] for rows in prob["views"]]
    got = host_calibrate(host, prob)
    assert got["ok"] and got["report"]["marker_state"] == [1, 1, 1, 1, 2, 2] and got["report"]["marker_rows"][4:] == [0, 0]
    assert got["report"]["markers_free"] == 4 and got["report"]["rows_used"] == 12 * 8
    for m in (4, 5):
        assert got["markers"][m].tobytes() == np.ascontiguousarray(prob["markers"][m]).tobytes()
        assert not got["cov"][m].any()
    assert min(got["cov"][m].diagonal().min() for m in range(4)) > 0
    wbb.check_against_witness(got, prob, "held markers")
    # the cascade (2 cameras): markers 0 - 3 in views 2 .. 11; view 0 holds markers {0, 4, 5} and view 1 {0, 1, 4}, both
    # cameras each; markers 4 and 5 are nowhere else.  Everything is free and used (marker 4 has 4 rows, marker 5 two).
    # Leave marker 4 one row (view 0, camera 0): it is held -> view 0 falls to the 2 distinct free markers {0, 5} ->
    # unused -> marker 5 has no row in a used view -> held.  (View 1 is left with {0, 1}: unused from the start.)
    prob = _rule_problem(rng, n_cam=2, n_mk=6)
    def cascade(whole):
        views = []
        for f, rows in enumerate(prob["views"]):
            if f == 0:
                views.append([r for r in rows if r[1] in (0, 5) or (r[1] == 4 and (whole or r[0] == 0))])
            elif f == 1:
                views.append([r for r in rows if r[1] in (0, 1) or (r[1] == 4 and whole)])
            else:
                views.append([r for r in rows if r[1] < 4])
        return dict(prob, views=views)
    # (all in, view 0 determines its pose and two markers from twelve numbers: the rules admit it, the geometry is the
    #  caller's concern — only what the rules decide is looked at, after one iteration)
    both = host_calibrate(host, cascade(True), max_iterations=1)
    assert both["report"]["marker_state"] == [1] * 6 and both["view_used"].all()
    assert both["report"]["marker_rows"][4:] == [4, 2] and both["report"]["rows_used"] == 6 + 6 + 10 * 8
    used_w, state_w, rows_w, two_w = wbb.plan(6, cascade(True)["views"])
    assert (list(both["view_used"]), both["report"]["marker_state"], both["report"]["marker_rows"]) == (used_w, state_w, rows_w)
    one = host_calibrate(host, cascade(False))
    assert one["ok"] and one["report"]["marker_state"] == [1, 1, 1, 1, 2, 2]
    assert list(one["view_used"]) == [False, False] + [True] * 10 and one["report"]["rows_used"] == 10 * 8
    for m in (4, 5):
        assert one["markers"][m].tobytes() == np.ascontiguousarray(prob["markers"][m]).tobytes()
    wbb.check_against_witness(one, cascade(False), "cascade, fallen")
    # fewer than 3 free markers: nothing is calibrated, everything comes back as given
    prob = _rule_problem(rng)
    prob["views"] = [[r for r in rows if r[1] < 2] for rows in prob["views"]]
    got = host_calibrate(host, prob)
    assert not got["ok"] and got["report"]["status"] == 1 and got["report"]["marker_state"] == [2] * 6
    assert got["report"]["views_used"] == 0 and got["report"]["markers_free"] == 0 and not got["view_used"].any()
    assert got["markers"].tobytes() == np.ascontiguousarray(prob["markers"]).tobytes()
    assert got["T_views"].tobytes() == np.ascontiguousarray(prob["T_start"]).tobytes() and not got["cov"].any()
    wbb.check_against_witness(got, prob, "two markers")


def test_rows_of_a_view_in_any_order(host):
    """The rows of every view shuffled: the same calibration within the criteria (the sums run in another order)."""
    rng = np.random.default_rng(13)
    prob = wbb.random_body_calibration(rng, 3, 15, 6)
    got = host_calibrate(host, prob)
    shuffled = dict(prob)
    shuffled["views"] = [[rows[i] for i in rng.permutation(len(rows))] for rows in prob["views"]]
    again = host_calibrate(host, shuffled)
    assert got["ok"] and again["ok"] and again["report"]["marker_rows"] == got["report"]["marker_rows"]
    assert np.abs(again["markers"] - got["markers"]).max() <= 1e-9 and np.abs(again["T_views"] - got["T_views"]).max() <= 1e-9
    wbb.check_against_witness(again, shuffled, "shuffled")


def test_scale_option_across_one_and_two_cameras(host):
    rng = np.random.default_rng(17)
    for n_cam in (1, 2):
        prob = wbb.random_body_calibration(rng, n_cam, 12, 5, p_missing=0.1)
        for scale, held in ((-1, n_cam == 1), (1, True)) + (((0, False),) if n_cam == 2 else ()):
            got = host_calibrate(host, prob, scale=scale)
            assert got["ok"] and got["report"]["scale_held"] == int(held), (n_cam, scale)
            wbb.check_against_witness(got, prob, (n_cam, scale), scale=scale)
            d0 = prob["markers"] - prob["markers"].mean(0)
            moved = got["markers"] - prob["markers"]
            if held:   # the size stays the start values' to first order: sum d . delta over the iterations
                assert abs((d0 * moved).sum()) <= 1e-3 * (d0 ** 2).sum(), (n_cam, scale)
            # the shape improves in either case (aligned with a similarity when the scale was held)
            assert wbb.shape_error(got["markers"], prob["markers_true"], held) < wbb.shape_error(prob["markers"], prob["markers_true"], held)
    # two cameras that never share a view: auto holds the scale
    prob = wbb.random_body_calibration(rng, 2, 12, 5, p_missing=0.0)
    prob["views"] = [[r for r in rows if r[0] == f % 2] for f, rows in enumerate(prob["views"])]
    got = host_calibrate(host, prob)
    assert got["ok"] and got["report"]["scale_held"] == 1
    wbb.check_against_witness(got, prob, "no shared view")


def test_the_inner_constraints_hold(host):
    """N^T (markers_out - markers_in): the translation components are sums of deltas that each satisfy sum delta_m = 0,
    so they vanish to rounding (<= 1e-12); the rotation and scale components are exact per iteration only about that
    iteration's centroid and d_m, so over the iterations they are second order in the step (a few mm): <= 1e-4 m^2."""
    rng = np.random.default_rng(19)
    for n_cam in (1, 3):
        prob = wbb.random_body_calibration(rng, n_cam, 10, 6, p_missing=0.1)
        got = host_calibrate(host, prob)
        assert got["ok"]
        N = wbb.gauge(np.asarray(prob["markers"], float), n_cam == 1)
        c = N.T @ (got["markers"] - prob["markers"]).reshape(-1)
        assert np.abs(c[:3]).max() <= 1e-12, c
        assert np.abs(c[3:]).max() <= 1e-4, c
        # one iteration: every component is a first-order zero
        one = host_calibrate(host, prob, max_iterations=1)
        c1 = N.T @ (one["markers"] - prob["markers"]).reshape(-1)
        assert np.abs(c1).max() <= 1e-12, c1


def test_iteration_cap_and_tolerance(host):
    rng = np.random.default_rng(23)
    prob = wbb.random_body_calibration(rng, 3, 10, 5)
    got = host_calibrate(host, prob, max_iterations=2)
    assert got["report"]["iterations"] == 2 and got["report"]["last_step"] > 1e-10
    wbb.check_against_witness(got, prob, "two iterations", max_iterations=2)
    loose = host_calibrate(host, prob, step_tolerance=1e-4)
    assert loose["report"]["iterations"] < host_calibrate(host, prob)["report"]["iterations"]


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", *flags, "-DBODY_BA_HOST_MAIN", *_extract(tmp_path), SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "body_ba_host ok:" in r.stdout, r.stdout
    return r.stdout


def test_body_ba_on_the_host_stand_alone(tmp_path):
    out = _build_and_run(tmp_path, "body_ba_host", ["-O2"])
    assert "up to 256 rows a view" in out and "bit for bit" in out, out


def test_body_ba_on_the_host_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "body_ba_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                  "-fno-omit-frame-pointer"])


C_USER = r"""
#include <stdio.h>
#include "mpe.h"
int main(void) {
  mpe_body_calibration_options opt;
  mpe_body_calibration_report rep;
  int (*cal)(mpe_handle*, const mpe_rig_camera*, int, const double*, int, const int*, const int*, const int*, const double*,
             int, const double*, const mpe_body_calibration_options*, double*, double*, double*, int*,
             mpe_body_calibration_report*) = mpe_body_calibrate;
  mpe_body_calibration_default_options(&opt);
  printf("%d %d %d %d %g %d\n", (int)sizeof(opt), (int)sizeof(rep), opt.scale, opt.max_iterations, opt.step_tolerance,
         cal != 0);
  return 0;
}
"""


def test_calibration_declarations_are_c99_exported_and_sized(tmp_path):
    mpe.build_library()
    lib = mpe.load_library()
    names = {"mpe_body_calibrate", "mpe_body_calibration_default_options"}
    assert names <= set(mpe.exported_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", mpe.library_path()], text=True)
    assert names <= set(re.findall(r" T (mpe_[a-z0-9_]+)", out))
    for n in names:
        assert getattr(lib, n).argtypes is not None, n
    src = tmp_path / "body_ba_user.c"
    src.write_text(C_USER)
    exe = str(tmp_path / "body_ba_user")
    libdir = os.path.dirname(mpe.library_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe, "-L", libdir, "-lmpe_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert got == [str(C.sizeof(mpe.MpeBodyCalibrationOptions)), str(C.sizeof(mpe.MpeBodyCalibrationReport)), "-1", "50", "1e-10",
                   "1"], got
    assert C.sizeof(mpe.MpeBodyCalibrationOptions) == 16 and C.sizeof(mpe.MpeBodyCalibrationReport) == 24 + 24 + 2 * 64
    # the refusals that need no device: a null handle is a usage error
    assert lib.mpe_body_calibrate(None, None, 1, None, 1, None, None, None, None, 0, None, None, None, None, None, None, None) == -1
