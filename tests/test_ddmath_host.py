"""csrc/mpe_ddmath.h — the device source of the libstdc++ / glibc restatement of std::pow(std::complex<double>, double)
(option "vote_arith" 3 / 4) — compiled for the HOST and held against THIS image's libm and libstdc++, the arithmetic
the CPU oracle runs on.  The literal restatements (glibc's hypot kernel, log1p, clog's branch structure) must agree bit
for bit; the correctly rounded primitives (log, exp, pow, atan2, sin, cos: double-double, rounded once) may differ from
glibc by one ulp where glibc itself misrounds — the rates are asserted, small, and printed.  Reference call sites:
p3p.cpp:262,264,268."""
import ctypes as C

import numpy as np
import pytest

from ddmath_cases import SPECIAL, beyond_cases, complex_cases, literal_cases, rounded_cases, special_grid
from host_builds import build_ddmath_host


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return build_ddmath_host(tmp_path_factory.mktemp("ddm_host"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _cmp(lib, which, a, b=None):
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(a if b is None else b, np.float64)
    m, l = np.zeros(len(a)), np.zeros(len(a))
    lib.ddm_compare(which, _p(a), _p(b), len(a), _p(m), _p(l))
    bad = ~((m == l) | (np.isnan(m) & np.isnan(l)))
    ulp = np.abs(m.view(np.int64) - l.view(np.int64))[bad]
    return float(bad.mean()), int(ulp.max()) if len(ulp) else 0


def test_literal_restatements_are_bit_exact(lib):
    """glibc's hypot kernel and its log1p are sequences of IEEE operations: restated, they must BE glibc's."""
    hyp, l1p = literal_cases()
    for a, b in hyp:
        assert _cmp(lib, 5, a, b) == (0.0, 0)
    for a in l1p:
        assert _cmp(lib, 8, a) == (0.0, 0)


@pytest.mark.parametrize("which,name,rate", [(0, "log", 2e-4), (2, "exp", 3e-3), (3, "sin", 5e-3), (4, "cos", 5e-3),
                                             (6, "atan2", 3e-3), (7, "pow", 3e-3)])
def test_correctly_rounded_primitives_agree_with_glibc_almost_everywhere(lib, which, name, rate):
    """Double-double evaluation rounded once against glibc (0.51 - 0.55 ulp): never more than one ulp apart, and apart
    only where glibc misrounds — measured here at 0.002 % (log) to 0.17 % (sin) of random arguments."""
    for a, b in rounded_cases(which):
        frac, ulp = _cmp(lib, which, a, b)
        print(name, "differs from glibc on %.4f %% of the arguments, by %d ulp at most" % (100 * frac, ulp))
        assert ulp <= 1 and frac <= rate, (name, frac, ulp)
    # special arguments take the library's own answers
    if which in (0, 2):
        assert _cmp(lib, which, SPECIAL) == (0.0, 0)
    if which == 6:
        assert _cmp(lib, 6, *special_grid()) == (0.0, 0)


@pytest.mark.parametrize("which,name,rate", [(3, "sin", 5e-3), (4, "cos", 5e-3), (6, "atan2", 3e-3)])
def test_no_library_call_where_the_operands_of_the_quartic_can_reach(lib, which, name, rate):
    """Angles between 1.1 and 3 pi_d, and magnitudes below 2^-500 or above 2^500 (subnormal operands of clog): evaluated
    by this header as well — quarter turns taken off in double-double, an exact rescaling — because the device's library is
    not glibc's.  Held to the same bounds against glibc as inside the ordinary range; on the few dozen hand-picked angles
    (the zeros of sine and cosine and their neighbours) the share of differing results says nothing — glibc misrounds
    cos(nextafter(pi_d / 2)), one ulp off the value 400-bit arithmetic gives — and the bound is the distance alone."""
    sets, picked = beyond_cases(which)
    for k, (a, b) in enumerate(sets + picked):
        frac, ulp = _cmp(lib, which, a, b)
        print(name, "beyond the ordinary range: differs from glibc on %.4f %% of %d arguments, by %d ulp at most" % (100 * frac, len(a), ulp))
        assert ulp <= 1 and (frac <= rate or k >= len(sets)), (name, frac, ulp)


def _ccmp(fn, re, im, *extra):
    re, im = np.ascontiguousarray(re, np.float64), np.ascontiguousarray(im, np.float64)
    m, l = np.zeros(2 * len(re)), np.zeros(2 * len(re))
    fn(_p(re), _p(im), *extra, len(re), _p(m), _p(l))
    bad = ~((m == l) | (np.isnan(m) & np.isnan(l)))
    ulp = np.abs(m.view(np.int64) - l.view(np.int64))[bad]
    return float(bad.reshape(-1, 2).any(1).mean()), int(ulp.max()) if len(ulp) else 0


def test_clog_and_complex_pow_against_libstdcxx(lib):
    """std::log(complex) = glibc clog through all of its branches (|z| far from 1: log(hypot); 1 < |x| < 2: log1p of
    (|x| - 1)(|x| + 1) + y^2; 0.5 <= |x| < 1: __x2y2m1; a real operand), and std::pow(complex, y) for the three exponents
    and the operand classes of p3p.cpp:262-268 (negative real with +0 / -0 imaginary part, positive real, general)."""
    c = complex_cases()
    for re, im in c["clog_general"]:
        frac, ulp = _ccmp(lib.ddm_clog, re, im)
        assert frac < 3e-3 and ulp <= 1, (frac, ulp)
    frac, ulp = _ccmp(lib.ddm_clog, *c["clog_negative_real"])
    assert frac < 2e-4 and ulp <= 1
    y = C.c_double(1 / 3.0)
    assert _ccmp(lib.ddm_cpow, *c["cpow_general"], y)[0] < 8e-3   # clog + exp + sincos: ~0.4 %
    for yv in (1 / 3.0, 2.0, 3.0):
        y = C.c_double(yv)
        for re, im in c["cpow_classes"]:
            frac, ulp = _ccmp(lib.ddm_cpow, re, im, y)
            assert frac < 3e-3 and ulp <= 8, (yv, frac, ulp)
    # pow(0, y) and NaN operands
    assert _ccmp(lib.ddm_cpow, *c["cpow_special"], C.c_double(1 / 3.0))[0] == 0.0
