"""CPU tier of the rig fusion: the logic of k_rig_refine (csrc/mpe_rig_gn.h) compiled for the host behind the tail helpers
of mpe_k3.hip (the `struct T34 {` .. `#define K3_GROUP` cut of test_geometry_host.py) and compared with a numpy witness
written in another formulation (tests/witness_rig.py: J = P R_c [I | -hat(X)], np.linalg.solve), with the criteria the
project applies to this refinement against its oracle (tests/test_gpu_parity.py:801-804): pose within 1e-9, covariance
allclose(rtol=1e-5, atol=1e-12), iteration counts within +-1.  One camera with the identity extrinsic must equal the host
build of k3_gauss_newton bit for bit.  The same source runs as a stand-alone program (own main) plain and under
AddressSanitizer + UndefinedBehaviorSanitizer, and the new declarations of include/mpe.h are checked: valid C99, exported,
ctypes sizes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rpg_monocular_pose_estimator_amd as mpe
import witness_rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "rig_gn_host.cpp")


def _extract(d):
    hip = mpe.device_source()
    i = hip.index("struct T34 {")
    with open(os.path.join(d, "k3_extract.inc"), "w") as fh:
        fh.write(hip[i:hip.index("#define K3_GROUP", i)])
    return ["-std=c++17", "-ffp-contract=off", "-I", str(d), "-I", os.path.join(ROOT, "tests", "host", "stub"), "-I", CSRC]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("rig_gn_host")
    so = os.path.join(d, "librig_gn_host.so")
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", *_extract(d), SRC, "-o", so])
    lib = C.CDLL(so)
    lib.host_rig_refine.restype = None
    lib.host_gauss_newton.restype = C.c_int
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_refine(host, cameras, rows, T0):
    cams = (mpe.MpeRigCamera * len(cameras))()
    for c, (K, E) in zip(cams, cameras):
        c.K[:] = np.asarray(K, float).reshape(9)
        c.T_cam_rig[:] = np.asarray(E, float).reshape(16)
    cam = np.ascontiguousarray([r[0] for r in rows], np.int32)
    xyz = np.ascontiguousarray([r[1] for r in rows], float).reshape(-1, 3)
    uv = np.ascontiguousarray([r[2] for r in rows], float).reshape(-1, 2)
    T0 = np.ascontiguousarray(T0, float)
    rec = np.zeros(1, mpe.RESULT_DTYPE)
    host.host_rig_refine(cams, len(cameras), _ptr(cam), _ptr(xyz), _ptr(uv), len(rows), _ptr(T0), _ptr(rec))
    return rec[0]


def test_rig_refinement_against_the_witness(host):
    rng = np.random.default_rng(2024)
    its = []
    for k in range(300):
        cameras, rows, T0 = witness_rig.random_rig(rng)
        rec = host_refine(host, cameras, rows, T0)
        assert rec["n_corr"] == len(rows) and rec["n_det"] == len({r[0] for r in rows}), k
        its.append(witness_rig.check_against_witness(rec, cameras, rows, T0, k))
    print("iterations per problem: %d .. %d" % (min(its), max(its)))
    assert 3 <= min(its) and max(its) <= 25, (min(its), max(its))


def test_one_camera_identity_is_k3_gauss_newton_bit_for_bit(host):
    rng = np.random.default_rng(7)
    for k in range(100):
        cameras, rows, T0 = witness_rig.random_rig(rng, n_cam=1)
        K = cameras[0][0]
        cameras = [(K, np.eye(4))]
        rec = host_refine(host, cameras, rows, T0)
        rows5 = np.ascontiguousarray([np.concatenate([r[1], r[2]]) for r in rows])
        k4 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
        T = np.ascontiguousarray(T0[:3, :])
        cov = np.zeros((6, 6))
        it = host.host_gauss_newton(_ptr(rows5), len(rows5), _ptr(k4), _ptr(T), _ptr(cov))
        assert it == rec["gn_iterations"], k
        assert T.tobytes() == rec["T"][:12].tobytes(), k
        assert cov.tobytes() == rec["cov"].tobytes(), k
        assert rec["status"] == 0 and list(rec["T"][12:]) == [0, 0, 0, 1]


def test_short_problems_have_no_pose(host):
    rng = np.random.default_rng(9)
    cameras, rows, T0 = witness_rig.random_rig(rng, n_cam=2)
    for n in (0, 1, 2):
        rec = host_refine(host, cameras, rows[:n], T0)
        assert rec["status"] == 1 and rec["gn_iterations"] == 0 and rec["n_corr"] == n
        assert np.array_equal(rec["T"].reshape(4, 4), T0) and not rec["cov"].any()


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", *flags, "-DRIG_GN_HOST_MAIN", *_extract(tmp_path), SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "rig_gn_host ok:" in r.stdout, r.stdout
    return r.stdout


def test_rig_gn_on_the_host_stand_alone(tmp_path):
    out = _build_and_run(tmp_path, "rig_gn_host", ["-O2"])
    assert "200 one-camera problems bit-equal" in out and "up to 256 rows" in out, out


def test_rig_gn_on_the_host_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "rig_gn_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                 "-fno-omit-frame-pointer"])


C_USER = r"""
#include <stdio.h>
#include "mpe.h"
int main(void) {
  mpe_rig_camera cam[MPE_RIG_MAX_CAMERAS];
  int (*batch)(mpe_handle*, const mpe_rig_camera*, int, const int*, const int*, const double*, const double*, int,
               const double*, mpe_result*) = mpe_rig_optimise_pose_batch;
  int (*fuse)(mpe_tracker* const*, int, const double*, const int*, mpe_result*, int*) = mpe_rig_fuse_trackers;
  int (*seed)(mpe_tracker* const*, int, const double*, const int*, const double[16], double, const double*, double) =
      mpe_rig_seed_trackers;
  printf("%d %d %d\n", (int)sizeof(cam[0]), (int)(sizeof(cam) / sizeof(cam[0])), batch && fuse && seed);
  return 0;
}
"""


def test_rig_declarations_are_c99_exported_and_sized(tmp_path):
    mpe.build_library()
    lib = mpe.load_library()
    names = {"mpe_rig_optimise_pose_batch", "mpe_rig_fuse_trackers", "mpe_rig_seed_trackers"}
    assert names <= set(mpe.exported_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", mpe.library_path()], text=True)
    assert names <= set(re.findall(r" T (mpe_[a-z0-9_]+)", out))
    for n in names:
        assert getattr(lib, n).argtypes is not None, n
    src = tmp_path / "rig_user.c"
    src.write_text(C_USER)
    exe = str(tmp_path / "rig_user")
    libdir = os.path.dirname(mpe.library_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe, "-L", libdir, "-lmpe_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert got == [str(C.sizeof(mpe.MpeRigCamera)), str(mpe.RIG_MAX_CAMERAS), "1"], got
    assert C.sizeof(mpe.MpeRigCamera) == (9 + 16) * 8
    # the refusals that need no device: a null handle or pointer is a usage error
    assert lib.mpe_rig_fuse_trackers(None, 0, None, None, None, None) == -1
    assert lib.mpe_rig_seed_trackers(None, 0, None, None, None, 0.0, None, 0.0) == -1
    assert lib.mpe_rig_optimise_pose_batch(None, None, 1, None, None, None, None, 0, None, None) == -1
