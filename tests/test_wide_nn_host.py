"""CPU tier of the wide tracked path: the nearest-neighbour correspondences of k_nn_wide (csrc/mpe_wide_nn.h) compiled
for the host as a stand-alone program (tests/host/wide_nn_host.cpp, own main) and run plain and under AddressSanitizer +
UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", CSRC] + flags +
                          [os.path.join(ROOT, "tests", "host", "wide_nn_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wide_nn_host ok:" in r.stdout, r.stdout
    return r.stdout


def test_wide_nn_on_the_host(tmp_path):
    """The 64-lane form (four detections per lane, butterfly reduction on (d2, index)) gives the rows of the plain double
    loop for 0 .. 256 detections x 1 .. 16 markers: random sets, exact ties in different lanes and in one lane,
    predictions exactly nn_tol away, NaN predictions and detections, two markers naming one detection; the compact
    record, the re-indexed rows and the slot table agree with the rows they were made from."""
    out = _build_and_run(tmp_path, "wide_nn_host", ["-O2"])
    w = out.split()
    sets, rows, ties, shared, edge = int(w[2]), int(w[4]), int(w[6]), int(w[8]), int(w[10])
    assert sets > 7000 and rows > 20000 and ties > 900 and shared > 100 and edge > 5000, out


def test_wide_nn_on_the_host_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "wide_nn_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
