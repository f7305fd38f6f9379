"""What tests/test_ddmath_device.py rests on, shown without a GPU.  csrc/mpe_ddmath.h is a sequence of IEEE + - * /
sqrt fma and exact scalings, so (a) a second correct compilation — ROCm's clang++, the front end and optimiser the
device build goes through, at the Makefile's -O3 -ffp-contract=off — has the bits of the g++ build on every selector
of csrc/mpe_ddmath_eval.h, the unrounded double-double pairs included; and (b) the comparison has teeth: a build that
may contract a * b + c differs on the literal restatements, while the correctly rounded primitives hide it."""
import ctypes as C

import numpy as np
import pytest

from ddmath_cases import eval_cases, special_grid
from host_builds import GXX, build_ddmath_host, rocm_clangxx

NAMES = ["log_cr", "log1p_cr", "exp_cr", "sin", "cos", "hypot_g", "atan2_cr", "pow_cr", "log1p_g", "clog_g", "cpow_g(1/3)",
         "cpow_g(2)", "cpow_g(3)", "csqrt_<true>", "x2y2m1_g", "two_prod", "add", "mul", "div", "sqrt_dd", "log_dd", "exp_dd",
         "atan_dd", "sin_dd", "cos_dd"]


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    d = tmp_path_factory.mktemp("ddm_builds")
    clang = rocm_clangxx()
    assert clang, "ROCm's clang++ not found (the compiler __graft_entry__.build() needs)"
    b = {"g++": build_ddmath_host(d, GXX, "libddm_gxx.so"),
         "clang++": build_ddmath_host(d, (clang, "-O3", "-ffp-contract=off"), "libddm_clang.so")}
    assert b["g++"].ddm_eval_count() == len(NAMES)
    if "fma" in open("/proc/cpuinfo").read().split():
        b["contracted"] = build_ddmath_host(d, (clang, "-O3", "-mfma", "-ffp-contract=fast"), "libddm_fma.so")
    return b


def _eval(lib, which, a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    out = np.zeros((len(a), 2))
    lib.ddm_eval(which, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), len(a), out.ctypes.data_as(C.c_void_p))
    return out


def _differing(x, y):
    same = (x.view(np.int64) == y.view(np.int64)) | (np.isnan(x) & np.isnan(y))
    return int((~same.all(1)).sum())


@pytest.mark.parametrize("which", range(len(NAMES)))
def test_a_second_compiler_gives_the_same_bits(builds, which):
    cases = eval_cases(which) + ([special_grid()] if which <= 18 else [])
    counts = [(len(a), _differing(_eval(builds["g++"], which, a, b), _eval(builds["clang++"], which, a, b))) for a, b in cases]
    print(NAMES[which], "clang++ -O3 against g++ -O1, both -ffp-contract=off (arguments, differing):", counts)
    assert all(d == 0 for _, d in counts), (NAMES[which], counts)


def test_the_comparison_notices_a_contracted_multiply_add(builds):
    """-mfma -ffp-contract=fast: hypot_g, log1p_g, clog_g and cpow_g differ from the uncontracted build; the counts of
    the correctly rounded primitives (0 when this was written: their one rounding hides the damage) and of the unrounded
    pairs are printed, not asserted."""
    if "contracted" not in builds:
        pytest.skip("this CPU has no FMA")
    counts = {}
    for which, name in enumerate(NAMES):
        a, b = eval_cases(which)[0]
        counts[name] = _differing(_eval(builds["g++"], which, a, b), _eval(builds["contracted"], which, a, b))
    print("results of %d arguments that a contracting build changes:" % len(a), counts)
    for name in ("hypot_g", "log1p_g", "clog_g", "cpow_g(1/3)", "cpow_g(2)", "cpow_g(3)"):
        assert counts[name] > 0, (name, counts)
