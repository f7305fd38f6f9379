"""CPU tier of the wide path (detection sets of 65 .. 256 points): the peel-and-compact logic of k3_peel_wide
(csrc/mpe_wide_peel.h) compiled for the host as a stand-alone program (tests/host/wide_peel_host.cpp, own main, the
oracle's shared library linked in) and run plain and under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")


def _build_and_run(orc, tmp_path, name, flags):
    exe = str(tmp_path / name)
    odir = os.path.join(ROOT, "oracle")   # (libmpe_oracle.so: built by the orc fixture, itself not instrumented)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC] + flags +
                          [os.path.join(ROOT, "tests", "host", "wide_peel_host.cpp"), "-o", exe, "-L", odir,
                           "-lmpe_oracle", "-Wl,-rpath," + odir])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wide_peel_host ok: 16001 histograms" in r.stdout, r.stdout
    return r.stdout


def test_wide_peel_on_the_host(orc, tmp_path):
    """correspondencesFromHistogram over 4 .. 256 x 4 .. 16 integer histograms (ties, duplicate rows, all-zero columns
    and tables, four thresholds each) equals the oracle's, the re-indexing into the compact record round-trips, a
    detection index of 256 survives, and the block table hands out every hypothesis of a 256 / 16 set once."""
    out = _build_and_run(orc, tmp_path, "wide_peel_host", ["-O2"])
    rows, shared = int(out.split()[4]), int(out.split()[6])
    assert rows > 20000 and shared > 500, out   # (the cases do name detections twice)


def test_wide_peel_on_the_host_under_sanitizers(orc, tmp_path):
    _build_and_run(orc, tmp_path, "wide_peel_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
