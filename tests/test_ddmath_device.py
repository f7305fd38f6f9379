"""csrc/mpe_ddmath.h as the DEVICE runs it (k_ddmath_batch / mpe_ddmath_batch, and variant 2 of k_quartic_batch), held
to the bits of its host build and to this machine's libm / libstdc++.

The header is a sequence of IEEE + - * / sqrt fma and exact scalings, so two correct compilations agree bit for bit:
criterion A compares the amdgcn build with the g++ build of the same source (tests/host/ddmath_host.cpp; both go
through ddm::eval of csrc/mpe_ddmath_eval.h) with an allowance of 0, on the literal restatements and the unrounded
double-double pairs as well — the final rounding of log_cr .. pow_cr hides a wrong last bit underneath it (a contracted
a * b + c changes none of them and 0.03 - 0.25 % of hypot_g / log1p_g / clog_g / cpow_g; tests/test_ddmath_builds_cpu.py
shows it).  Criterion B
holds the device results to the bounds tests/test_ddmath_host.py asserts for the host build against the library."""
import ctypes as C

import numpy as np
import pytest

from ddmath_cases import SPECIAL, beyond_cases, complex_cases, eval_cases, literal_cases, rounded_cases, special_grid, tiny_cases
from host_builds import build_ddmath_host, build_geom_host
from util import check_quartic_roots, quartic_test_problems, unstable_quartic_problems

pytestmark = pytest.mark.gpu

MPE_ERR_ARG = -1
NAMES = ["log_cr", "log1p_cr", "exp_cr", "sin", "cos", "hypot_g", "atan2_cr", "pow_cr", "log1p_g", "clog_g", "cpow_g(1/3)",
         "cpow_g(2)", "cpow_g(3)", "csqrt_<true>", "x2y2m1_g", "two_prod", "add", "mul", "div", "sqrt_dd", "log_dd", "exp_dd",
         "atan_dd", "sin_dd", "cos_dd"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = build_ddmath_host(tmp_path_factory.mktemp("ddm_host"))
    assert lib.ddm_eval_count() == len(NAMES)
    return lib


@pytest.fixture(scope="module")
def geom(tmp_path_factory):
    return build_geom_host(tmp_path_factory.mktemp("geom_host"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_eval(host, which, a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    out = np.zeros((len(a), 2))
    host.ddm_eval(which, _p(a), _p(b), len(a), _p(out))
    return out


def _differing(x, y):
    """Rows that are not bit-equal, a NaN equal to a NaN."""
    same = (x.view(np.int64) == y.view(np.int64)) | (np.isnan(x) & np.isnan(y))
    return ~same.reshape(len(x), -1).all(1)


def _against_library(m, l):
    """(share of arguments whose result differs from the library's, largest distance in ulp), as test_ddmath_host.py
    counts them; m, l: (n,) or (n, 2)."""
    bad = ~((m == l) | (np.isnan(m) & np.isnan(l)))
    ulp = np.abs(m.view(np.int64) - l.view(np.int64))[bad]
    return float(bad.reshape(len(m), -1).any(1).mean()), int(ulp.max()) if len(ulp) else 0


def _lib_real(host, which, a, b=None):
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(a if b is None else b, np.float64)
    m, l = np.zeros(len(a)), np.zeros(len(a))
    host.ddm_compare(which, _p(a), _p(b), len(a), _p(m), _p(l))
    return l


def _lib_complex(fn, re, im, *extra):
    re, im = np.ascontiguousarray(re, np.float64), np.ascontiguousarray(im, np.float64)
    m, l = np.zeros((len(re), 2)), np.zeros((len(re), 2))
    fn(_p(re), _p(im), *extra, len(re), _p(m), _p(l))
    return l


# ---- criterion A: the device build against the host build of the same source, allowance 0 -----------------------------
@pytest.mark.parametrize("which", range(len(NAMES)))
def test_device_build_has_the_bits_of_the_host_build(hip, host, which):
    """Every argument set of the selector (those of test_ddmath_host.py at 200 000 arguments each, the subnormal and
    near-DBL_MIN operands of hypot_g / clog_g, the sets of the selectors this file is the first to reach) and, for the
    functions defined on them, every pair of +-0, +-inf, NaN, +-1: both outputs, bit for bit."""
    cases = eval_cases(which)
    if which <= 18:   # (the *_dd functions from sqrt_dd on are defined on positive normal / bounded operands only)
        cases = cases + [special_grid()]
    counts = []
    for a, b in cases:
        dev = hip.ddmath_batch(which, a, b)
        counts.append((len(a), int(_differing(dev, _host_eval(host, which, a, b)).sum())))
    print(NAMES[which], "device results differing from the host build's (arguments, differing):", counts)
    assert all(d == 0 for _, d in counts), (NAMES[which], counts)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_tail_lanes_and_block_boundaries(hip, host, n):
    """One lane per argument in blocks of 64: a batch of one, one short of a block, a block, one over — every selector,
    and nothing written behind the batch's results."""
    for which in range(len(NAMES)):
        a, b = eval_cases(which)[0]
        a, b = a[:n], b[:n]
        dev = hip.ddmath_batch(which, a, b)
        assert dev.shape == (n, 2) and not _differing(dev, _host_eval(host, which, a, b)).any(), (NAMES[which], n)


# ---- criterion B: the device results against this machine's libm / libstdc++, with the host build's bounds ------------
def test_device_literal_restatements_are_the_librarys_bits(hip, host):
    """hypot_g and log1p_g on the device ARE glibc's hypot and log1p: 0 differing (the bound of
    test_literal_restatements_are_bit_exact), the subnormal operands of hypot's scaling branch included."""
    hyp, l1p = literal_cases()
    res = []
    for a, b in hyp + tiny_cases():
        res.append(("hypot_g",) + _against_library(hip.ddmath_batch(5, a, b)[:, 0], _lib_real(host, 5, a, b)))
    for a in l1p:
        res.append(("log1p_g",) + _against_library(hip.ddmath_batch(8, a)[:, 0], _lib_real(host, 8, a)))
    print("device against libm (function, share differing, ulp):", res)
    assert all(r[1:] == (0.0, 0) for r in res), res


@pytest.mark.parametrize("which,name,rate", [(0, "log", 2e-4), (2, "exp", 3e-3), (3, "sin", 5e-3), (4, "cos", 5e-3),
                                             (6, "atan2", 3e-3), (7, "pow", 3e-3)])
def test_device_rounded_primitives_agree_with_glibc_almost_everywhere(hip, host, which, name, rate):
    """The bounds of test_correctly_rounded_primitives_agree_with_glibc_almost_everywhere: at most one ulp from glibc,
    on at most `rate` of the arguments; the special arguments take the library's own answers."""
    res = []
    for a, b in rounded_cases(which):
        res.append(_against_library(hip.ddmath_batch(which, a, b)[:, 0], _lib_real(host, which, a, b)))
        print(name, "on the device differs from glibc on %.4f %% of the arguments, by %d ulp at most" % (100 * res[-1][0], res[-1][1]))
    assert all(ulp <= 1 and frac <= rate for frac, ulp in res), (name, res)
    if which in (0, 2):
        assert _against_library(hip.ddmath_batch(which, SPECIAL)[:, 0], _lib_real(host, which, SPECIAL)) == (0.0, 0)
    if which == 6:
        a, b = special_grid()
        assert _against_library(hip.ddmath_batch(6, a, b)[:, 0], _lib_real(host, 6, a, b)) == (0.0, 0)


@pytest.mark.parametrize("which,name,rate", [(3, "sin", 5e-3), (4, "cos", 5e-3), (6, "atan2", 3e-3)])
def test_device_rounded_primitives_beyond_the_ordinary_range(hip, host, which, name, rate):
    """The bounds of test_no_library_call_where_the_operands_of_the_quartic_can_reach: angles up to 3 pi_d, magnitudes
    below 2^-500 and above 2^500 (on these the header once called the platform's library, which on the device is not
    glibc's: clog_g of subnormal operands and cpow_g(z, 2), cpow_g(z, 3) of a general z differed from the host build)."""
    sets, picked = beyond_cases(which)
    res = [_against_library(hip.ddmath_batch(which, a, b)[:, 0], _lib_real(host, which, a, b)) for a, b in sets + picked]
    print(name, "on the device beyond the ordinary range (share differing from glibc, ulp):", res)
    assert all(ulp <= 1 for _, ulp in res) and all(frac <= rate for frac, _ in res[:len(sets)]), (name, res)


def test_device_clog_and_complex_pow_against_libstdcxx(hip, host):
    """The fractions and ulp caps of test_clog_and_complex_pow_against_libstdcxx, for the device's clog_g and cpow_g."""
    c = complex_cases()
    res = {}
    for k, (re, im) in enumerate(c["clog_general"]):
        res["clog", k] = _against_library(hip.ddmath_batch(9, re, im), _lib_complex(host.ddm_clog, re, im))
    re, im = c["clog_negative_real"]
    res["clog", "negative real"] = _against_library(hip.ddmath_batch(9, re, im), _lib_complex(host.ddm_clog, re, im))
    re, im = c["cpow_general"]
    res["cpow", "general"] = _against_library(hip.ddmath_batch(10, re, im), _lib_complex(host.ddm_cpow, re, im, C.c_double(1 / 3.0)))
    for which, yv in ((10, 1 / 3.0), (11, 2.0), (12, 3.0)):
        for k, (re, im) in enumerate(c["cpow_classes"]):
            res["cpow", yv, k] = _against_library(hip.ddmath_batch(which, re, im), _lib_complex(host.ddm_cpow, re, im, C.c_double(yv)))
    for k, (re, im) in enumerate(tiny_cases()):   # (subnormal operands: the bounds of clog's general operand)
        res["clog", "tiny", k] = _against_library(hip.ddmath_batch(9, re, im), _lib_complex(host.ddm_clog, re, im))
    re, im = c["cpow_special"]
    res["cpow", "special"] = _against_library(hip.ddmath_batch(10, re, im), _lib_complex(host.ddm_cpow, re, im, C.c_double(1 / 3.0)))
    print("device against libstdc++ (share differing, ulp):", res)
    for k in range(3):
        assert res["clog", k][0] < 3e-3 and res["clog", k][1] <= 1, res
    for k in range(len(tiny_cases())):
        assert res["clog", "tiny", k][0] < 3e-3 and res["clog", "tiny", k][1] <= 1, res
    assert res["clog", "negative real"][0] < 2e-4 and res["clog", "negative real"][1] <= 1, res
    assert res["cpow", "general"][0] < 8e-3, res
    for yv in (1 / 3.0, 2.0, 3.0):
        for k in range(3):
            assert res["cpow", yv, k][0] < 3e-3 and res["cpow", yv, k][1] <= 8, res
    assert res["cpow", "special"][0] == 0.0, res


# ---- the glibc-faithful quartic (variant 2: solve_quartic_glibc, the function the strict voting item calls) ------------
def test_device_quartic_with_glibc_powers(hip, geom, orc):
    """On the 20 000 quartics of test_glibc_powers_put_the_quartic_on_the_oracles_digits and on quartic_test_problems(2):
    bit-equal to the host build of solve_quartic<true>; against the oracle within that test's bounds (at most 0.3 %
    differing bitwise, at most 4 beyond 1e-9); and through check_quartic_roots."""
    f = np.ascontiguousarray(unstable_quartic_problems())
    f2, roots2 = quartic_test_problems(2)
    f2 = np.ascontiguousarray(f2)
    dev, dev2 = hip.solve_quartic_batch(f, 2), hip.solve_quartic_batch(f2, 2)
    for ff, d in ((f, dev), (f2, dev2)):
        want = np.zeros((len(ff), 4))
        geom.host_quartic(_p(ff), len(ff), 2, _p(want))
        n_diff = int(_differing(d, want).sum())
        print("device quartics differing from the host build's: %d of %d" % (n_diff, len(ff)))
        assert n_diff == 0
    ref = np.array([orc.solve_quartic(f[i]) for i in range(len(f))])
    same = (dev == ref) | (np.isnan(dev) & np.isnan(ref))
    res = (int((~same.all(1)).sum()), int((np.abs(dev - ref).max(1) > 1e-9).sum()))
    print("device quartics differing from the oracle (bitwise, beyond 1e-9):", res)
    assert res[0] <= 0.003 * len(f) and res[1] <= 4, res
    check_quartic_roots(dev2, f2, roots2, orc)


# ---- usage errors ------------------------------------------------------------------------------------------------------
def test_usage_errors_leave_the_handle_usable(hip, host):
    lib, h = hip._lib, hip._h
    a = np.linspace(0.5, 2.0, 7)
    out = np.zeros((7, 2))
    f, r = np.ones((1, 5)), np.zeros((1, 4))
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    null = C.POINTER(C.c_double)()
    assert lib.mpe_ddmath_batch(h, -1, dp(a), dp(a), 7, dp(out)) == MPE_ERR_ARG
    assert lib.mpe_ddmath_batch(h, len(NAMES), dp(a), dp(a), 7, dp(out)) == MPE_ERR_ARG
    assert lib.mpe_ddmath_batch(h, 0, null, dp(a), 7, dp(out)) == MPE_ERR_ARG
    assert lib.mpe_ddmath_batch(h, 0, dp(a), null, 7, dp(out)) == MPE_ERR_ARG
    assert lib.mpe_ddmath_batch(h, 0, dp(a), dp(a), 7, null) == MPE_ERR_ARG
    assert lib.mpe_ddmath_batch(h, 0, dp(a), dp(a), -1, dp(out)) == MPE_ERR_ARG
    assert lib.mpe_solve_quartic_batch(h, dp(f), 1, 3, dp(r)) == MPE_ERR_ARG
    assert lib.mpe_solve_quartic_batch(h, dp(f), 1, -1, dp(r)) == MPE_ERR_ARG
    assert not out.any() and not r.any()
    assert lib.mpe_ddmath_batch(h, 0, null, null, 0, null) == 0     # n == 0: nothing to do
    assert hip.ddmath_batch(0, []).shape == (0, 2)
    assert not _differing(hip.ddmath_batch(0, a), _host_eval(host, 0, a, a)).any()
    assert np.isfinite(hip.solve_quartic_batch(f, 2)).all()
