"""Known-answer tests that pin the CPU oracle (oracle/) — the reference has no tests of its own.
CPU only.  Each block cites what it pins in the reference."""
import itertools

import numpy as np
import pytest

import witness
from rpg_monocular_pose_estimator_amd import synth

RNG = np.random.default_rng(12345)


# ---- Combinations (combinations.cpp) ---------------------------------------------------------
def test_combinations_tables(orc):
    assert orc.combinations3(4).tolist() == [[1, 2, 3], [1, 2, 4], [1, 3, 4], [2, 3, 4]]
    c5 = orc.combinations3(5)
    assert c5.tolist() == [list(c) for c in itertools.combinations(range(1, 6), 3)]
    for n, cnt in [(4, 4), (5, 10), (8, 56), (12, 220)]:
        c = orc.combinations3(n)
        assert len(c) == cnt and c.tolist() == sorted(c.tolist())
        assert c.tolist() == [list(x) for x in itertools.combinations(range(1, n + 1), 3)]


def test_permutation_blocks(orc):
    # combinations.cpp:205-244 permutations(3) = [3 2 1],[3 1 2],[2 3 1],[2 1 3],[1 2 3],[1 3 2],
    # applied as indices to every lexicographic combination (combinations.cpp:131-203)
    p4 = orc.permutations3(4)
    assert len(p4) == 24
    assert p4[:6].tolist() == [[3, 2, 1], [3, 1, 2], [2, 3, 1], [2, 1, 3], [1, 2, 3], [1, 3, 2]]
    assert p4[6:12].tolist() == [[4, 2, 1], [4, 1, 2], [2, 4, 1], [2, 1, 4], [1, 2, 4], [1, 4, 2]]
    for n, cnt in [(5, 60), (8, 336)]:
        p = orc.permutations3(n)
        assert len(p) == cnt
        assert len({tuple(r) for r in p.tolist()}) == cnt  # all rows distinct
        assert {tuple(r) for r in p.tolist()} == set(itertools.permutations(range(1, n + 1), 3))


def test_num_combinations_32bit_factorial_quirk(orc):
    assert [orc.num_combinations(n, 3) for n in (4, 5, 8, 12)] == [4, 10, 56, 220]
    # combinations.cpp:34-45: unsigned 32-bit factorial overflows from 13! on; replicated
    f13 = (6227020800) % (1 << 32)
    assert orc.num_combinations(13, 3) == f13 // (6 * 3628800) == 88


# ---- quartic / P3P (p3p.cpp) -------------------------------------------------------------------
def test_quartic_four_real_roots(orc):
    for _ in range(200):
        roots = np.sort(RNG.uniform(-2, 2, 4))
        if np.min(np.diff(roots)) < 0.05:
            continue
        a = RNG.uniform(0.5, 2) * RNG.choice([-1, 1])
        coef = a * np.poly(roots)
        got = np.sort(orc.solve_quartic(coef))
        assert np.allclose(got, roots, atol=1e-8), (roots, got)


def test_quartic_complex_roots_real_parts(orc):
    # p3p.cpp:276-283 takes .real() of complex roots: check against mpmath
    for _ in range(100):
        re1, im1 = RNG.uniform(-1, 1), RNG.uniform(0.2, 1)
        r3, r4 = RNG.uniform(-2, 2, 2)
        if abs(r3 - r4) < 0.1:
            continue
        coef = np.real(np.poly([re1 + 1j * im1, re1 - 1j * im1, r3, r4])) * RNG.uniform(0.5, 2)
        got = np.sort(orc.solve_quartic(coef))
        ref = np.sort([z.real for z in witness.quartic_roots_mp(coef)])
        assert np.allclose(got, ref, atol=1e-7), (got, ref)


def _random_pose(rng):
    T = np.eye(4)
    T[:3, :3] = synth.rodrigues(rng.normal(size=3), rng.uniform(0, 1.0))
    T[:3, 3] = [rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), rng.uniform(0.8, 2.5)]
    return T


def test_p3p_round_trip(orc):
    """One of the 4 solutions [R|C] is the inverse of the true T_camera_object (p3p.cpp:50,226-232)."""
    K = synth.README_K
    for _ in range(50):
        T = _random_pose(RNG)
        W = synth.M5[RNG.permutation(5)[:3]]
        pc = (T[:3, :3] @ W.T).T + T[:3, 3]
        F = pc / np.linalg.norm(pc, axis=1, keepdims=True)
        rc, sol = orc.p3p(F, W)
        assert rc == 0
        Tinv = np.linalg.inv(T)
        errs = [np.abs(s - Tinv[:3, :]).max() for s in sol if np.all(np.isfinite(s))]
        assert min(errs) < 1e-8, errs
        # every finite solution has an orthonormal R; solutions built from the real part of a
        # COMPLEX quartic root (quirk A.6.6) are still rigid transforms, just not P3P solutions
        for s in sol:
            if np.all(np.isfinite(s)):
                assert np.allclose(s[:, :3] @ s[:, :3].T, np.eye(3), atol=1e-9)


def test_p3p_collinear_returns_minus_one(orc):
    W = np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0]])
    F = np.array([[0, 0, 1.0], [0.1, 0, 1], [0.2, 0, 1]])
    F /= np.linalg.norm(F, axis=1, keepdims=True)
    assert orc.p3p(F, W)[0] == -1


# ---- pose primitives (pose_estimator.cpp) ------------------------------------------------------
def test_image_vectors_and_project2d(orc):
    K = synth.README_K
    det = RNG.uniform(50, 400, (6, 2))
    v = orc.image_vectors(det, K)
    assert np.allclose(np.linalg.norm(v, axis=1), 1)
    assert np.allclose(v[:, 0] / v[:, 2], (det[:, 0] - K[0, 2]) / K[0, 0])
    T = _random_pose(RNG)
    p = np.array([0.05, -0.02, 0.1, 1.0])
    assert np.allclose(orc.project2d(p, T, K), witness.project(T, p[:3], K), atol=1e-10)


def test_exponential_map_matches_expm(orc):
    assert np.array_equal(orc.exponential_map(np.zeros(6)), np.eye(4))
    for _ in range(30):
        tw = RNG.normal(size=6) * RNG.choice([1e-8, 1e-3, 0.5, 2.0])
        E = orc.exponential_map(tw)
        assert np.allclose(E, witness.se3_exp(tw), atol=1e-9)
        assert np.allclose(E[:3, :3] @ E[:3, :3].T, np.eye(3), atol=1e-12)


def test_jacobian_finite_differences(orc):
    # pose_estimator.cpp:945-957: d project(exp(eps) T p) / d eps at eps = 0, twist = (upsilon, omega)
    K = synth.README_K
    for _ in range(10):
        T = _random_pose(RNG)
        p = np.append(RNG.uniform(-0.1, 0.1, 3), 1.0)
        J = orc.jacobian(T, p, K[0, 0], K[1, 1])
        Jn = np.zeros((2, 6))
        h = 1e-6
        for i in range(6):
            e = np.zeros(6)
            e[i] = h
            Jn[:, i] = (witness.project(witness.se3_exp(e) @ T, p[:3], K) -
                        witness.project(witness.se3_exp(-e) @ T, p[:3], K)) / (2 * h)
        assert np.allclose(J, Jn, rtol=1e-5, atol=1e-4)


def test_kabsch(orc):
    for _ in range(20):
        T = _random_pose(RNG)
        A = synth.M8
        B = (T[:3, :3] @ A.T).T + T[:3, 3]
        Tk = orc.compute_transformation(A, B)
        assert np.allclose(Tk, T, atol=1e-10)
        R, t = witness.kabsch(A, B + RNG.normal(size=B.shape) * 1e-3)
    # noisy case agrees with numpy's SVD route
    Bn = B + RNG.normal(size=B.shape) * 1e-3
    R, t = witness.kabsch(A, Bn)
    Tk = orc.compute_transformation(A, Bn)
    assert np.allclose(Tk[:3, :3], R, atol=1e-10) and np.allclose(Tk[:3, 3], t, atol=1e-10)


def test_gauss_newton_converges_to_truth(orc):
    K = synth.README_K
    for _ in range(10):
        T = _random_pose(RNG)
        M = synth.M5
        det = np.array([witness.project(T, m, K) for m in M])
        corr = np.array([[i + 1, i + 1] for i in range(5)], np.uint32)
        T0 = witness.se3_exp(RNG.normal(size=6) * 0.02) @ T
        Topt, cov, it = orc.optimise_pose(det, M, K, corr, T0)
        assert it <= 12
        assert np.allclose(Topt, T, atol=1e-9)
        assert np.allclose(cov, cov.T, rtol=1e-6, atol=1e-15) and np.all(np.linalg.eigvalsh(cov) > 0)


def test_correspondences_from_histogram_semantics(orc):
    # pose_estimator.cpp:344-370: column-major first maximum, only the COLUMN is zeroed, stop below threshold
    h = np.array([[5, 0, 9], [9, 2, 9], [1, 9, 0]], np.uint32)
    c = orc.correspondences_from_histogram(h, 2)
    # first max 9 in column-major order is (row 1, col 0) -> marker 1 / detection 2; then col 1 (row 2); then col 2 (row 0)
    assert c.tolist() == [[1, 2], [2, 3], [3, 1]]
    # one detection may serve several markers (quirk A.6.7)
    h2 = np.array([[7, 8], [0, 0]], np.uint32)
    assert orc.correspondences_from_histogram(h2, 1).tolist() == [[2, 1], [1, 1]]
    assert len(orc.correspondences_from_histogram(h, 10)) == 0


# ---- LED detection (led_detector.cpp + OpenCV semantics) ---------------------------
def test_gaussian_kernel_quantisation(orc):
    assert orc.gaussian_kernel_q8(0.6).tolist() == [1, 42, 170, 42, 1]
    for s in (0.3, 0.6, 0.85, 1.0, 1.7, 2.5, 6.0):
        assert orc.gaussian_kernel_q8(s).tolist() == witness.gaussian_taps_q8(s).tolist()
    with pytest.raises(ValueError):
        orc.gaussian_kernel_q8(0.0)


def test_blur_matches_numpy_witness(orc):
    for (h, w, sigma) in [(40, 50, 0.6), (7, 9, 0.6), (33, 17, 1.2), (5, 5, 0.6), (64, 64, 0.3)]:
        img = RNG.integers(0, 256, (h, w)).astype(np.uint8)
        b, m = orc.blur_mask(img, 140, sigma)
        ref = witness.blur_fixed_point(img, 140, sigma)
        assert np.array_equal(b, ref)
        assert np.array_equal(m, (ref != 0).astype(np.uint8))


def test_threshold_is_strict(orc):
    img = np.zeros((9, 9), np.uint8)
    img[4, 4] = 140
    assert orc.blur_mask(img, 140, 0.6)[1].sum() == 0   # == threshold is NOT kept (quirk A.6.3)
    img[4, 4] = 141
    assert orc.blur_mask(img, 140, 0.6)[1].sum() > 0


def test_single_bright_pixel_dilation(orc):
    # a lone 255: the 5x5 fixed-point kernel leaves a plus-shaped support
    img = np.zeros((11, 11), np.uint8)
    img[5, 5] = 255
    _, m = orc.blur_mask(img, 140, 0.6)
    exp = np.zeros((11, 11), np.uint8)
    exp[4:7, 4:7] = 1
    exp[3, 5] = exp[7, 5] = exp[5, 3] = exp[5, 7] = 1
    assert np.array_equal(m, exp)


def _mask(rows):
    return np.array([[1 if ch == "#" else 0 for ch in r] for r in rows], np.uint8)


def test_contours_hand_drawn(orc):
    # 1 pixel
    c = orc.external_contours(_mask(["...", ".#.", "..."]))
    assert len(c) == 1 and c[0].tolist() == [[1, 1]]
    # 2x2 square: start top-left, first step goes down (counter-clockwise on screen)
    c = orc.external_contours(_mask(["....", ".##.", ".##.", "...."]))
    assert c[0].tolist() == [[1, 1], [1, 2], [2, 2], [2, 1]]
    # 3x3 square: 8 border pixels, polygon area 4
    c = orc.external_contours(_mask([".....", ".###.", ".###.", ".###.", "....."]))
    assert c[0].tolist() == [[1, 1], [1, 2], [1, 3], [2, 3], [3, 3], [3, 2], [3, 1], [2, 1]]
    assert witness.shoelace(c[0]) == 4.0
    # plus shape
    c = orc.external_contours(_mask([".....", "..#..", ".###.", "..#..", "....."]))
    assert c[0].tolist() == [[2, 1], [1, 2], [2, 3], [3, 2]]
    # horizontal 1-px line: pixels of the interior appear twice (there and back)
    c = orc.external_contours(_mask([".....", ".###.", "....."]))
    assert c[0].tolist() == [[1, 1], [2, 1], [3, 1], [2, 1]]
    # diagonal line
    c = orc.external_contours(_mask(["#...", ".#..", "..#.", "...#"]))
    assert c[0].tolist() == [[0, 0], [1, 1], [2, 2], [3, 3], [2, 2], [1, 1]]
    # two squares touching by a corner are ONE 8-connected component
    c = orc.external_contours(_mask(["##..", "##..", "..##", "..##"]))
    assert len(c) == 1
    # blob touching the border is kept (image is zero-padded by one pixel)
    c = orc.external_contours(_mask(["##.", "##.", "..."]))
    assert len(c) == 1 and c[0].tolist() == [[0, 0], [0, 1], [1, 1], [1, 0]]


def test_contour_order_and_nesting(orc):
    # order: newest first (the last component met in raster order is contours[0])
    m = _mask(["#....", ".....", "..#..", ".....", "....#"])
    c = orc.external_contours(m)
    assert [x[0].tolist() for x in c] == [[4, 4], [2, 2], [0, 0]]
    # RETR_EXTERNAL: a blob inside the hole of a ring is not reported; one outside is
    ring = _mask(["#######..", "#.....#..", "#..#..#.#", "#.....#..", "#######.."])
    c = orc.external_contours(ring)
    starts = sorted(tuple(x[0]) for x in c)
    assert starts == [(0, 0), (8, 2)]


def test_component_count_matches_scipy(orc):
    from scipy import ndimage
    for _ in range(10):
        m = (RNG.random((40, 60)) > 0.8).astype(np.uint8)
        lab, n = ndimage.label(m, structure=np.ones((3, 3)))
        c = orc.external_contours(m)
        # every component that is not enclosed by another one has exactly one external contour
        fill = ndimage.binary_fill_holes(m)
        _, n_top = ndimage.label(fill, structure=np.ones((3, 3)))
        assert len(c) == n_top <= n
        for pts in c:
            assert all(m[y, x] for x, y in pts)


def test_find_leds_centroid_is_polygon_centroid(orc):
    # quirk A.6.1: the centroid is that of the contour POLYGON (cv::moments on the point list)
    K, D = synth.README_K, np.zeros(5)
    rng = np.random.default_rng(3)
    img = synth.render_frame(rng, np.array([[100.3, 80.6]]), 160, 200)
    P = orc.make_params()
    und, dist = orc.find_leds(img, P, K, D)
    assert len(dist) == 1
    _, m = orc.blur_mask(img, 140, 0.6)
    c = orc.external_contours(m)
    assert len(c) == 1
    assert np.allclose(dist[0], witness.polygon_centroid(c[0]).astype(np.float32), atol=1e-5)
    assert np.linalg.norm(dist[0] - [100.3, 80.6]) < 0.5
    assert np.allclose(und, dist, atol=1e-4)  # no distortion, P = K: identity up to float32


def test_find_leds_filter_integer_halves(orc):
    # quirk A.6.2: std::pow(rect.width / 2, 2) uses INTEGER division: a 5x5 polygon (area 16)
    # is tested against pi*2^2, not pi*2.5^2
    K, D = synth.README_K, np.zeros(5)
    img = np.zeros((40, 40), np.uint8)
    img[10:13, 10:13] = 255   # 3x3 bright -> blurred support 7x7 minus corners
    P = orc.make_params(min_blob_area=1, max_blob_area=1000, max_circular_distortion=0.6)
    und, dist = orc.find_leds(img, P, K, D)
    _, m = orc.blur_mask(img, 140, 0.6)
    c = orc.external_contours(m)[0]
    w = c[:, 0].max() - c[:, 0].min() + 1
    area = witness.shoelace(c)
    keep = abs(1 - area / (np.pi * (w // 2) ** 2)) <= 0.6
    assert (len(dist) == 1) == keep


def test_undistort_inverts_distort(orc):
    K, D = synth.README_K, synth.README_D
    pts = np.stack([RNG.uniform(100, 650, 20), RNG.uniform(60, 420, 20)], 1).astype(np.float32)
    d = orc.distort_points(pts, K, D)
    assert np.allclose(d, synth.distort_px(pts, K, D), atol=1e-3)
    u = orc.undistort_points(d, K, D)
    assert np.abs(u - pts).max() < 0.05   # 5 fixed-point iterations, float32 output


# A 15 x 11 grid of ideal pixel positions that covers the 752 x 480 image; what the camera sees of them is the forward
# rational model written out in detection_parameter_cases.forward_rational.
def _image_grid():
    gx, gy = np.meshgrid(np.linspace(0, 751, 15), np.linspace(0, 479, 11))
    return np.stack([gx.ravel(), gy.ravel()], 1)


# largest |undistort(forward(p)) - p| (Euclidean, px) of the oracle over that grid, measured on the development machine
# (five fixed-point iterations do not converge further; the corners decide):
INVERSION_ERROR_PX = {"README": 0.0821, "D4": 0.0821, "D5": 0.1859, "D8": 0.2333, "D12": 0.2333}


@pytest.mark.parametrize("name", ["D0", "README", "D4", "D5", "D8", "D12"])
def test_undistort_with_0_4_5_8_coefficients(orc, name):
    """cv::undistortPoints' rational model k1 k2 p1 p2 k3 k4 k5 k6 (led_detector.h:81: 4, 5 or 8 coefficients) in the
    oracle: bit for bit the independent witness (tests/witness_pipeline.py) for every coefficient count, and the inverse
    of the forward rational model written out in plain float64 to within TWICE the error measured for that camera
    (INVERSION_ERROR_PX above: 0.082 px README and D4, 0.186 px D5, 0.233 px D8 and D12; no distortion: float32 rounding
    alone).  Coefficients beyond the eighth are ignored."""
    import detection_parameter_cases as dpc
    import witness_pipeline
    K, D = dpc.CAMERAS[name]
    grid = _image_grid()
    seen = dpc.forward_rational(grid, K, D).astype(np.float32)
    und = orc.undistort_points(seen, K, D)
    assert np.array_equal(und, witness_pipeline.undistort_points(seen, K, D))
    err = float(np.linalg.norm(und - grid, axis=1).max())
    print("inversion error", name, err)
    assert err <= (2 * INVERSION_ERROR_PX[name] if len(D) else 1e-4), (name, err)
    if name == "D12":
        assert np.array_equal(und, orc.undistort_points(seen, K, dpc.D8))
    if name == "D4":
        assert np.array_equal(und, orc.undistort_points(seen, K, synth.README_D))   # README's k3 is 0.0


def test_undistort_uses_every_coefficient_of_the_rational_model(orc):
    """Zeroing any one of the eight coefficients of D8 moves some grid point by more than 0.1 px (k3 k4 k5 k6 alone:
    2.2, 115, 8.3 and 0.35 px): an answer that matches the witness has used that coefficient."""
    import detection_parameter_cases as dpc
    K = synth.README_K
    seen = dpc.forward_rational(_image_grid(), K, dpc.D8).astype(np.float32)
    und = orc.undistort_points(seen, K, dpc.D8)
    for i in range(8):
        D = dpc.D8.copy()
        D[i] = 0.0
        assert np.linalg.norm(orc.undistort_points(seen, K, D) - und, axis=1).max() > 0.1, i


def test_distort_points_ignores_k4_k5_k6(orc):
    """LEDDetector::distortPoints is polynomial only (led_detector.cpp:190-194): k1 k2 p1 p2 k3, whatever else D holds;
    missing coefficients are zero.  Oracle, witness and the library's host arithmetic agree bit for bit."""
    import detection_parameter_cases as dpc
    import witness_pipeline
    import rpg_monocular_pose_estimator_amd as mpe
    grid = _image_grid().astype(np.float32)
    for name, (K, D) in dpc.CAMERAS.items():
        d = orc.distort_points(grid, K, D)
        assert np.array_equal(d, np.array(witness_pipeline.distort_points(grid, K, D), np.float32)), name
        assert np.array_equal(d, mpe.distort_points(grid, K, D)), name
        assert np.array_equal(d, orc.distort_points(grid, K, (list(D) + [0.0] * 5)[:5])), name
        roi = orc.determine_roi(grid[20:25], 480, 752, 20, K, D)
        assert roi == witness_pipeline.determine_roi(grid[20:25], 480, 752, 20, K, D) == \
            tuple(mpe.determine_roi(grid[20:25], 480, 752, 20, K, D)), name


def test_roi_detection_offsets(orc):
    d = synth.make_frames("C2", 1, seed=5)
    P = orc.make_params()
    full_u, full_d = orc.find_leds(d["frames"][0], P, d["K"], d["D"])
    s = d["spots"][0]
    roi = (int(s[:, 0].min() - 30), int(s[:, 1].min() - 30), int(np.ptp(s[:, 0]) + 60), int(np.ptp(s[:, 1]) + 60))
    roi = (max(roi[0], 0), max(roi[1], 0), min(roi[2], 752 - max(roi[0], 0)), min(roi[3], 480 - max(roi[1], 0)))
    ru, rd = orc.find_leds(d["frames"][0], P, d["K"], d["D"], roi=roi)
    assert len(ru) == len(full_u) == 5
    assert np.allclose(rd, full_d, atol=1e-4)


# ---- whole path ---------------------------------------------------------------------------------
def test_vote_histogram_true_correspondences_dominate(orc):
    K = synth.README_K
    T = _random_pose(np.random.default_rng(2))
    det = np.array([witness.project(T, m, K) for m in synth.M5])
    h = orc.vote_histogram(det, synth.M5, K, 5.0)
    assert h.shape == (5, 5)
    assert np.all(np.diag(h) >= 10)          # every true pair collects >= C(5,3) votes
    assert np.all(np.argmax(h, axis=0) == np.arange(5))


def test_end_to_end_synthetic_pose_accuracy(orc):
    d = synth.make_frames("C2", 24, seed=1234)
    res = orc.estimate_batch(d["frames"], d["markers"], d["K"], d["D"], orc.make_params(), n_threads=4)
    ok = res["status"] == 0
    assert ok.sum() >= 18
    err = [np.linalg.norm(res["T"][i].reshape(4, 4)[:3, 3] - d["T_true"][i][:3, 3]) for i in np.nonzero(ok)[0]]
    assert np.median(err) < 5e-3 and np.max(err) < 5e-2   # polygon-centroid bias ~0.2 px
    assert np.all(res["n_det"] == 5)
    it = res["gn_iterations"][ok]
    assert it.min() >= 3 and it.max() <= 12


def test_fewer_than_four_leds_gives_no_pose(orc):
    K, D = synth.camera_for(480, 752)
    rng = np.random.default_rng(0)
    img = synth.render_frame(rng, np.array([[100.5, 100.2], [300.1, 200.7], [500.9, 400.3]]), 480, 752)
    r = orc.estimate_batch(img[None], synth.M5, K, D, orc.make_params())
    assert r["status"][0] == 1 and r["n_det"][0] == 3 and r["n_corr"][0] == 0


# ---- tracking path (pose_estimator.cpp:232-244, 372-392, 996-1064; led_detector.cpp:114-179) ----
def test_logarithm_map_inverts_exponential_map(orc):
    from scipy.linalg import logm
    assert np.array_equal(orc.logarithm_map(np.eye(4)), np.zeros(6))
    for _ in range(30):
        tw = RNG.normal(size=6) * RNG.choice([1e-6, 1e-2, 0.3, 1.0])
        T = witness.se3_exp(tw)
        xi = orc.logarithm_map(T)
        assert np.allclose(xi, tw, atol=1e-9), (xi, tw)
        L = np.real(logm(T))
        assert np.allclose(xi[:3], L[:3, 3], atol=1e-8)
        assert np.allclose(xi[3:], [L[2, 1], L[0, 2], L[1, 0]], atol=1e-8)
    # pure translation: w = 0 -> A_inv = I
    T = np.eye(4)
    T[:3, 3] = [0.1, -0.2, 0.3]
    assert np.allclose(orc.logarithm_map(T), [0.1, -0.2, 0.3, 0, 0, 0])


def test_tracker_state_machine(orc):
    d = synth.make_sequence("C2", 24, seed=3, dropout=(10, 11))
    tr = orc.Tracker(d["markers"], d["K"], d["D"], orc.make_params())
    rs = [tr.estimate(d["frames"][k], d["times"][k]) for k in range(24)]
    assert rs[0]["updated"] and rs[0]["used_bruteforce"] and rs[0]["roi"] == (0, 0, 752, 480)
    assert rs[0]["it_since_initialized"] == 1 and rs[1]["it_since_initialized"] == 2
    for k in range(1, 10):   # ROI tracking: small ROI around the LEDs (+20 px border), no brute force
        assert rs[k]["updated"] and not rs[k]["used_bruteforce"]
        x, y, w, h = rs[k]["roi"]
        assert w < 200 and h < 200
        px = d["T_true"][k]
        assert rs[k]["n_corr"] == 5
    for k in (10, 11):       # 2 LEDs only: ROI search fails, whole image retried, no pose
        assert not rs[k]["updated"] and rs[k]["roi"] == (0, 0, 752, 480) and rs[k]["n_det"] == 2
    assert rs[12]["updated"]  # recovers (prediction from the last two poses still lands on the LEDs)
    for k in range(24):
        if rs[k]["updated"]:
            assert np.linalg.norm(rs[k]["T"][:3, 3] - d["T_true"][k][:3, 3]) < 0.03


def test_reference_ferrari_is_unstable_when_w_vanishes(orc):
    """A well-conditioned quartic taken from a real hypothesis (tests/data/vote_regression_det_0.npy,
    detections 0,2,3 <-> markers 3,2,1) on which the reference's Ferrari formulas (p3p.cpp:238-286) lose
    ~14 digits: alpha + 2y ~ 0 makes w tiny and 2*beta/w huge.  The literal restatement is off by 1.7e-2
    from the true roots, and a 1-ulp change of one coefficient moves its answer by > 1e-4 — so in such
    (rare, ~1e-7 of all hypotheses) cases no two builds of the reference agree with each other, and the
    HIP path cannot be vote-identical either."""
    F = np.array([-2.6726739687181578, 0.16730140900912122, 2.3718487024017842, -0.14465695719931068,
                  0.17769794483556164])
    true = np.sort([z.real for z in witness.quartic_roots_mp(F)])
    got = np.sort(orc.solve_quartic(F))
    assert np.allclose(true, [-0.97555999, 0.02847635, 0.02847635, 0.98120430], atol=1e-7)
    assert 5e-3 < np.abs(got - true).max() < 5e-2          # the reference algorithm itself is this far off
    moved = 0.0
    for k in range(5):
        for sgn in (-1, 1):
            G = F.copy()
            G[k] = np.nextafter(G[k], sgn * np.inf)
            moved = max(moved, np.abs(np.sort(orc.solve_quartic(G)) - got).max())
    assert moved > 1e-4                                     # 1 ulp in -> 1e-4 .. 1e-2 out


def test_blur_formulations_across_opencv_generations(orc):
    """Which OpenCV the blur semantics restate, and where it matters.  The oracle / witness /
    kernels restate generation A (OpenCV <= 3.4.1: getGaussianKernel(CV_32F) -> 8-bit integer taps, 8u32s filter
    engine).  Against the two later data paths of cv::GaussianBlur for CV_8U (tests/witness.py):
      * B (3.4.2 .. 4.1.1, ufixedpoint16, taps rounded from the CV_64F kernel): the SAME taps for every sigma on a 0.01
        grid over (0, 6] (the dynamic-reconfigure range, cfg:13), and the same non-zero mask on images that drive the
        16-bit horizontal accumulator into saturation;
      * C (>= 4.1.2, error-diffused taps that sum to exactly 256): the same taps at the demo / default sigma 0.6 — the
        only value the launch files and the cfg default use — but different taps at most other sigmas, i.e. there a
        build of the reference against OpenCV 4 produces another mask than one against OpenCV 3.3, and this restatement
        follows the latter."""
    rng = np.random.default_rng(12)
    sig = np.round(np.arange(1, 601) * 0.01, 2)
    differs_c = []
    for s in sig:
        a = witness.gaussian_taps_q8(float(s))
        assert np.array_equal(a, witness.gaussian_taps_ufixedpoint16(float(s))), s
        assert np.array_equal(a, np.asarray(orc.gaussian_kernel_q8(float(s)))), s
        if not np.array_equal(a, witness.gaussian_taps_bitexact_ed(float(s))):
            differs_c.append(float(s))
    assert 0.6 not in differs_c and 1.0 not in differs_c
    assert 450 <= len(differs_c) <= 560, len(differs_c)   # most of the grid
    # generation B's saturating 8.8 accumulator does not change the MASK (only plateau values of the blurred image)
    for s in (0.3, 0.6, 0.77, 1.5, 3.1, 6.0):
        img = rng.integers(0, 31, (64, 96)).astype(np.uint8)
        img[20:40, 30:70] = 255                      # a plateau that saturates 255 * sum(taps) when sum(taps) > 257
        img[5, 5] = 200
        img[50:52, 80:83] = 180
        taps = witness.gaussian_taps_q8(s)
        m_a = witness.blur_mask_generation(img, 140, taps, False)
        m_b = witness.blur_mask_generation(img, 140, taps, True)
        assert np.array_equal(m_a, m_b), s
        assert np.array_equal(m_a, witness.blur_fixed_point(img, 140, s) != 0), s
        _, m_orc = orc.blur_mask(img, 140, s)
        assert np.array_equal(m_a, np.asarray(m_orc) != 0), s
    # ... and generation C really is another function where its taps differ: a sigma with a visible difference
    n_diff_px = 0
    for s in differs_c[:60]:
        img = np.zeros((40, 40), np.uint8)
        img[18:22, 18:22] = rng.integers(141, 256, (4, 4))
        m_a = witness.blur_mask_generation(img, 140, witness.gaussian_taps_q8(s), False)
        m_c = witness.blur_mask_generation(img, 140, witness.gaussian_taps_bitexact_ed(s), True)
        n_diff_px += int((m_a != m_c).sum())
    assert n_diff_px > 0


def test_convert_to_mono8_restates_cv_bridge(orc):
    """cv_bridge::toCvCopy(msg, MONO8) (monocular_pose_estimator.cpp:147): BGR / RGB(A) -> gray with OpenCV's 14-bit
    integer coefficients, mono16 -> mono8 by convertTo(CV_8U, 255 / 65535.) in single precision, round half to even —
    against independent numpy forms, incl. the known values 255/255/255 -> 255, pure channels, 65535 -> 255."""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (9, 13, 3)).astype(np.uint8)
    y = (img[..., 0].astype(np.int64) * 1868 + img[..., 1].astype(np.int64) * 9617 + img[..., 2].astype(np.int64) * 4899
         + (1 << 13)) >> 14
    assert np.array_equal(orc.convert_to_mono8(img, "bgr8"), y.astype(np.uint8))
    assert np.array_equal(orc.convert_to_mono8(img[..., ::-1], "rgb8"), y.astype(np.uint8))
    img4 = np.concatenate([img, rng.integers(0, 256, (9, 13, 1)).astype(np.uint8)], axis=2)
    assert np.array_equal(orc.convert_to_mono8(img4, "bgra8"), y.astype(np.uint8))
    assert np.array_equal(orc.convert_to_mono8(np.ascontiguousarray(img4[..., [2, 1, 0, 3]]), "rgba8"), y.astype(np.uint8))
    px = np.array([[[255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [0, 0, 0]]], np.uint8)
    assert orc.convert_to_mono8(px, "bgr8").tolist() == [[255, 29, 150, 76, 0]]   # 0.114 / 0.587 / 0.299 of 255
    m = rng.integers(0, 65536, (6, 7)).astype(np.uint16)
    ref = np.clip(np.rint(m.astype(np.float32) * np.float32(255. / 65535.)), 0, 255).astype(np.uint8)
    assert np.array_equal(orc.convert_to_mono8(m, "mono16"), ref)
    assert np.array_equal(orc.convert_to_mono8(m.byteswap(), "mono16", big_endian=True), ref)
    assert orc.convert_to_mono8(np.array([[65535, 0, 257, 128, 129]], np.uint16), "mono16").tolist() == [[255, 0, 1, 0, 1]]
    g = rng.integers(0, 256, (4, 5)).astype(np.uint8)
    assert np.array_equal(orc.convert_to_mono8(g, "mono8"), g)
