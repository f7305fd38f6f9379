"""The argument sets of the mpe_ddmath.h tests, stated once: tests/test_ddmath_host.py runs them through the host build
against libm / libstdc++, tests/test_ddmath_device.py through the device build against the host build and libm."""
import numpy as np

N = 200000
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0])
DBL_MIN = 2.2250738585072014e-308


def literal_cases():
    """-> (hypot_g argument pairs, log1p_g arguments): magnitudes over e^+-10, nearly equal legs, one leg zero, both
    legs scaled to 1e-200 and 1e200 (hypot's scaling branches); log1p_g through every interval of its polynomial."""
    rng = np.random.default_rng(1)
    x = rng.normal(size=N) * np.exp(rng.uniform(-10, 10, N))
    y = rng.normal(size=N) * np.exp(rng.uniform(-10, 10, N))
    hyp = [(x, y), (x, x * rng.uniform(0.5, 2, N)), (x, np.zeros(N)), (x * 1e-200, y * 1e-200), (x * 1e200, y * 1e200)]
    l1p = [rng.uniform(-0.99, 3, N), rng.uniform(-1e-5, 1e-5, N), rng.uniform(-1e-10, 1e-10, N),
           np.exp(rng.uniform(-5, 40, N)), rng.uniform(-0.30, 0.42, N), np.array([0.0, -0.0, -1.0, -2.0, np.inf, np.nan])]
    return hyp, l1p


def rounded_cases(which):
    """Argument pairs (a, b or None) of the correctly rounded primitive `which` (0 log, 2 exp, 3 sin, 4 cos, 6 atan2,
    7 pow)."""
    rng = np.random.default_rng(2 + which)
    if which == 0:
        return [(np.exp(rng.uniform(-40, 40, N)), None), (1 + rng.uniform(-1e-3, 1e-3, N), None)]
    if which == 2:
        return [(rng.uniform(-60, 60, N), None), (rng.uniform(-1e-3, 1e-3, N), None)]
    if which in (3, 4):
        return [(rng.uniform(-1.1, 1.1, N), None)]
    if which == 6:
        return [(rng.normal(size=N), rng.normal(size=N)),
                (rng.normal(size=N) * np.exp(rng.uniform(-10, 10, N)), rng.normal(size=N) * np.exp(rng.uniform(-10, 10, N)))]
    x = np.exp(rng.uniform(-40, 40, N))
    return [(x, np.full(N, 1 / 3.0)), (x, np.full(N, 3.0)), (x, np.full(N, 2.0))]


def special_grid():
    """Every pair of SPECIAL: (a, b), 49 pairs."""
    yy, xx = np.meshgrid(SPECIAL, SPECIAL)
    return yy.ravel(), xx.ravel()


def complex_cases():
    """Operands (re, im) of clog and pow(complex, y): clog's three magnitude classes (|z| over e^+-12, within e^+-0.7 of
    the unit circle, on it) and a negative real; for the powers a general operand and the operand classes of
    p3p.cpp:262-268 (negative real with +0 / -0 imaginary part, positive real); pow(0, y) and a NaN."""
    rng = np.random.default_rng(9)
    ang = rng.uniform(-np.pi, np.pi, N)
    c = {"clog_general": [(mag * np.cos(ang), mag * np.sin(ang))
                          for mag in (np.exp(rng.uniform(-12, 12, N)), np.exp(rng.uniform(-0.7, 0.7, N)), np.ones(N))]}
    c["clog_negative_real"] = (-np.exp(rng.uniform(-30, 5, N)), np.zeros(N))
    mag = np.exp(rng.uniform(-12, 12, N))
    c["cpow_general"] = (mag * np.cos(ang), mag * np.sin(ang))
    c["cpow_classes"] = [(-mag, np.zeros(N)), (-mag, -np.zeros(N)), (mag, np.zeros(N))]
    c["cpow_special"] = (np.array([0.0, -0.0, np.nan]), np.zeros(3))
    return c


def pair_cases(which):
    """Argument pairs of the selectors the host tests never reached on their own (csrc/mpe_ddmath_eval.h): the quartic's
    complex square root (13), __x2y2m1 (14) and the unrounded double-double pairs (15 - 24), each inside the domain its
    function documents."""
    rng = np.random.default_rng(100 + which)
    wide = lambda: rng.normal(size=N) * np.exp(rng.uniform(-10, 10, N))
    if which == 13:     # both half-planes, the real axis with +0 / -0, nearly real and nearly imaginary operands
        x, y = wide(), wide()
        return [(x, y), (x, np.zeros(N)), (x, -np.zeros(N)), (x, x * 1e-12 * rng.normal(size=N)), (y * 1e-12, x)]
    if which == 14:     # 0.5 <= x < 1, x^2 + y^2 >= 0.5: the operands clog hands it, and beyond
        ang = rng.uniform(0, np.pi / 4, N)
        mag = np.exp(rng.uniform(-0.3, 0.3, N))
        return [(mag * np.cos(ang), mag * np.sin(ang)), (np.cos(ang), np.sin(ang)), (rng.uniform(0.5, 1, N), rng.uniform(0, 1, N))]
    if which in (15, 16, 17, 18):   # any finite operands; nearly equal and nearly opposite ones for the cancellations
        x = wide()
        return [(x, wide()), (x, x * (1 + rng.normal(size=N) * 1e-9)), (x, -x * (1 + rng.normal(size=N) * 1e-9)),
                (x * 1e-150, wide() * 1e-150)]
    if which in (19, 20):           # x = a b > 0 and normal
        return [(np.abs(wide()), np.abs(wide())), (np.exp(rng.uniform(-300, 300, N)), np.exp(rng.uniform(-300, 300, N))),
                (1 + rng.uniform(-1e-3, 1e-3, N), 1 + rng.uniform(-1e-3, 1e-3, N))]
    if which == 21:                 # |a b| < 700
        return [(rng.uniform(-26, 26, N), rng.uniform(-26, 26, N)), (rng.uniform(-1e-3, 1e-3, N), rng.uniform(-1, 1, N))]
    if which == 22:                 # a b in [0, 1]
        return [(rng.uniform(0, 1, N), rng.uniform(0, 1, N)), (np.exp(rng.uniform(-30, 0, N)), rng.uniform(0, 1, N))]
    assert which in (23, 24), which  # |a| <= pi
    return [(rng.uniform(-np.pi, np.pi, N), None), (rng.uniform(-1.1, 1.1, N), None), (rng.uniform(-1e-6, 1e-6, N), None)]


def beyond_cases(which):
    """Arguments beyond the range of rounded_cases on which sin / cos (3, 4) and atan2 (6) once answered with the
    platform library's function — which on the device is not glibc's: angles up to 3 pi_d (y arg z for y = 2, 3 and a
    general z; the zeros of sine and cosine and their neighbours, where a relative error shows), and magnitudes below
    2^-500 or above 2^500 — subnormal, huge, one of each, and quotients on both sides of the 2^-400 below which atan t
    rounds as t.  -> (random sets, hand-picked sets)."""
    rng = np.random.default_rng(40 + which)
    n = 20000
    if which in (3, 4):
        pi_d = 3.141592653589793
        t = rng.choice([-1.0, 1.0], N) * rng.uniform(1.1, 3 * pi_d, N)
        q = 0.5 * pi_d * np.arange(1, 7)   # the zeros of the cosine and of the sine, and their neighbours
        edge = np.concatenate([q, np.nextafter(q, 0), np.nextafter(q, 10), 0.25 * pi_d * np.arange(3, 12, 2), [1.1, np.nextafter(1.1, 2)]])
        return [(t, None)], [(np.concatenate([edge, -edge]), None)]
    assert which == 6, which
    wide = lambda: rng.normal(size=n) * np.exp(rng.uniform(-10, 10, n))
    c = tiny_cases()
    c += [(wide() * 1e200, wide() * 1e200), (wide() * 1e-200, wide() * 1e200), (wide() * 1e200, wide() * 1e-200),
          (wide() * 1e-130, wide() * 1e-10), (wide() * 1e-10, wide() * 1e-130), (wide() * 1e-160, wide() * 1e-290),
          (wide() * 5e-324, wide()), (wide(), wide() * 5e-324)]
    return c, []


def eval_cases(which):
    """Every argument set of selector `which`, as pairs (a, b): what the device build is held to the host build on."""
    def both(cases):
        return [(a, a if b is None else b) for a, b in cases]
    if which in (3, 4, 6):
        return both(rounded_cases(which) + sum(beyond_cases(which), []))
    if which in (0, 2, 7):
        return both(rounded_cases(which))
    hyp, l1p = literal_cases()
    if which in (1, 8):
        return both((a, None) for a in l1p)
    if which == 5:
        return hyp + tiny_cases()
    c = complex_cases()
    if which == 9:
        return c["clog_general"] + [c["clog_negative_real"]] + tiny_cases()
    if which in (10, 11, 12):
        return [c["cpow_general"]] + c["cpow_classes"] + [c["cpow_special"]]
    return both(pair_cases(which))


def tiny_cases():
    """Subnormal and near-DBL_MIN operand pairs for hypot_g and clog_g (the scaling branch of clog when both parts are
    below DBL_MIN, hypot's when the smaller leg is): both subnormal, one subnormal beside a small normal, both within
    a factor 4 of DBL_MIN, and the smallest subnormals."""
    rng = np.random.default_rng(21)
    n = 20000
    sgn = lambda: rng.choice([-1.0, 1.0], n)
    sub = lambda: sgn() * DBL_MIN * rng.uniform(0, 1, n)
    near = lambda: sgn() * DBL_MIN * rng.uniform(0.25, 4, n)
    few = lambda: sgn() * 5e-324 * rng.integers(0, 9, n)
    return [(sub(), sub()), (sub(), near()), (near(), sub()), (near(), near()), (few(), few()), (near(), few())]
