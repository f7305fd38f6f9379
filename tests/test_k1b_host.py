"""The DEVICE source of the blob extraction (threshold, fixed-point blur, Suzuki border following, polygon sums,
shape filter, undistortion: everything of K1b that is not wave plumbing), compiled for the HOST and checked against
the oracle's findLeds — the CPU tier has no GPU, but it can still run the very code the GPU runs.

The region is cut out of the kernel sources (rpg_monocular_pose_estimator_amd/csrc/mpe_k1.hip; binding.device_source) at test time (tests/host/k1b_host.cpp
holds the one-lane shims and the whole-frame flow of the device's general tier).  Reference being matched:
led_detector.cpp:35-112 through oracle.find_leds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rpg_monocular_pose_estimator_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")


def _cut(text, begin, end):
    i = text.index(begin)
    return text[i:text.index(end, i)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("k1b_host")
    import rpg_monocular_pose_estimator_amd as mpe
    hip = mpe.device_source()
    internal = open(os.path.join(CSRC, "mpe_internal.h")).read()
    with open(os.path.join(d, "k1a_extract.inc"), "w") as fh:
        fh.write(_cut(hip, "struct ThrTest {", "#ifndef K1A_UNROLL"))
    inc = _cut(internal, "struct DetectParams {", "struct SolveParams {")
    inc += _cut(hip, "struct BlobRec {", "// final stage: kept blobs")
    with open(os.path.join(d, "k1b_extract.inc"), "w") as fh:
        fh.write(inc)
    so = os.path.join(d, "libk1b_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", *os.environ.get("MPE_HOST_CXXFLAGS", "").split(), "-I", str(d),
                           os.path.join(ROOT, "tests", "host", "k1b_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.host_find_leds.restype = C.c_int
    return lib


def _host_find_leds(lib, orc, img, P, K, D, roi_xy=(0, 0)):
    taps = np.ascontiguousarray(orc.gaussian_kernel_q8(P.gaussian_sigma), np.int32)
    shape = np.array([P.min_blob_area, P.max_blob_area, P.max_width_height_distortion, P.max_circular_distortion])
    Kf = np.ascontiguousarray(np.asarray(K, float).reshape(9))
    Df = np.ascontiguousarray(np.asarray(D, float).reshape(-1))
    cap = 4096
    dist = np.zeros((cap, 2), np.float32)
    und = np.zeros((cap, 2))
    img = np.ascontiguousarray(img, np.uint8)
    n = lib.host_find_leds(img.ctypes.data_as(C.c_void_p), img.shape[0], img.shape[1], int(P.threshold_value),
                           taps.ctypes.data_as(C.c_void_p), len(taps), shape.ctypes.data_as(C.c_void_p),
                           Kf.ctypes.data_as(C.c_void_p), Df.ctypes.data_as(C.c_void_p), len(Df), roi_xy[0], roi_xy[1],
                           dist.ctypes.data_as(C.c_void_p), und.ctypes.data_as(C.c_void_p), cap)
    assert n >= 0
    return und[:n], dist[:n]


@pytest.fixture(scope="module")
def orc():
    import oracle
    oracle.build()
    from oracle import binding
    return binding


def _random_image(rng, rows, cols, kind):
    img = rng.integers(0, 60, (rows, cols)).astype(np.uint8)  # below the threshold
    if kind == "spots":  # LED-like Gaussian spots, some on the border (mirrored blur taps)
        yy, xx = np.mgrid[0:rows, 0:cols]
        for _ in range(rng.integers(1, 9)):
            cx, cy = rng.uniform(-2, cols + 2), rng.uniform(-2, rows + 2)
            s = rng.uniform(0.8, 4.0)
            img = np.maximum(img, (255 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))).astype(np.uint8))
    elif kind == "noise":  # salt: single pixels, thin lines, touching components, holes after the blur
        m = rng.random((rows, cols)) < rng.uniform(0.01, 0.2)
        img[m] = rng.integers(100, 256, m.sum())
    else:  # rings and bars: nested components and holes (RETR_EXTERNAL must skip what lies inside)
        yy, xx = np.mgrid[0:rows, 0:cols]
        for _ in range(rng.integers(1, 5)):
            cx, cy, r = rng.uniform(0, cols), rng.uniform(0, rows), rng.uniform(5, 30)
            d = np.hypot(xx - cx, yy - cy)
            for rr in np.arange(r, 4, -rng.uniform(6, 9)):  # concentric rings ...
                img[(d > rr - 1.5) & (d < rr + 1.0)] = 255
            if rng.random() < 0.7:
                img[(d < 1.8)] = 230                         # ... around a disc
        if rng.random() < 0.5:
            y0 = rng.integers(0, rows)
            img[y0:y0 + 1, rng.integers(0, cols // 2):] = 200
    return img


@pytest.mark.parametrize("kind", ["spots", "noise", "rings"])
def test_device_blob_source_on_the_host_equals_the_oracle(host, orc, kind):
    rng = np.random.default_rng({"spots": 1, "noise": 2, "rings": 3}[kind])
    n_blobs = 0
    for it in range(400):
        rows, cols = int(rng.integers(8, 90)), int(rng.integers(18, 150))
        img = _random_image(rng, rows, cols, kind)
        K, D = synth.camera_for(rows, cols)
        if it % 3 == 0:  # wide-open shape filter: every traced contour with a non-degenerate box is reported
            P = orc.make_params(min_blob_area=0.0, max_blob_area=1e9, max_width_height_distortion=1e9,
                                max_circular_distortion=1e9, gaussian_sigma=[0.6, 0.5, 0.85, 0.2][it % 12 // 3])  # 5, 3, 7 taps; [0, 256, 0]
        else:
            P = orc.make_params(gaussian_sigma=0.6 if it % 2 else 0.4)
        roi_xy = (int(rng.integers(0, 50)), int(rng.integers(0, 50))) if it % 4 == 1 else (0, 0)
        # (the oracle adds the ROI origin of the window it is given; here the window is the whole small image and the
        #  origin is only the float offset of led_detector.cpp:74)
        ref_und, ref_dist = orc.find_leds(np.pad(img, ((roi_xy[1], 0), (roi_xy[0], 0))), P, K, D,
                                          roi=(roi_xy[0], roi_xy[1], cols, rows))
        und, dist = _host_find_leds(host, orc, img, P, K, D, roi_xy)
        assert len(dist) == len(ref_dist), (kind, it, len(dist), len(ref_dist))
        assert np.array_equal(dist, ref_dist, equal_nan=True), (kind, it)   # float32 centroids, bit for bit, same order
        # (a zero-area contour that the wide-open filter lets through has a 0 / 0 centroid on both sides)
        assert np.array_equal(und, ref_und, equal_nan=True), (kind, it)     # undistorted: float32 stored as double
        n_blobs += len(dist)
    assert n_blobs > 100, n_blobs


def test_blurred_value_exactly_at_the_rounding_boundary(host, orc):
    """GaussianBlur keeps a pixel iff (sum + 2^15) >> 16 != 0, i.e. sum >= 2^15.  With taps [1, 42, 170, 42, 1] three dim
    pixels (1 at the output position, 2 one step diagonally, 2 two steps to the side) give exactly
    170*170 + 2*42*42 + 2*170 = 32768; the mask pixel they switch on touches the halo of a bright block three pixels
    away, so it changes that blob's contour and centroid: '>=' and '>' give different answers."""
    img = np.zeros((40, 48), np.uint8)
    img[10:20, 10:20] = 255              # its blurred mask reaches x = 21 (two pixels beyond the block)
    y, x = 15, 22                        # diagonal neighbour of the halo: 8-connected to the blob
    img[y, x] = 1
    img[y + 1, x + 1] = 2
    img[y, x + 2] = 2
    K, D = synth.camera_for(40, 48)
    P = orc.make_params(threshold_value=0, gaussian_sigma=0.6, min_blob_area=0.0, max_blob_area=1e9,
                        max_width_height_distortion=1e9, max_circular_distortion=1e9)
    assert list(orc.gaussian_kernel_q8(0.6)) == [1, 42, 170, 42, 1]
    blurred, mask = orc.blur_mask(img, 0, 0.6)
    assert mask[y, x] and not mask[y - 1, x] and not mask[y + 1, x]   # the bridge between the halo and (y, x + 1)
    ref_und, ref_dist = orc.find_leds(img, P, K, D)
    und, dist = _host_find_leds(host, orc, img, P, K, D)
    assert len(ref_dist) == 1 and np.array_equal(dist, ref_dist) and np.array_equal(und, ref_und)
    img[y, x] = 0                                      # below the boundary: the bridge is gone and the answer changes
    _, dist2 = _host_find_leds(host, orc, img, P, K, D)
    assert not np.array_equal(dist2, dist)


def test_scan_threshold_arithmetic_exhaustively(host):
    """The image scan flags a 16-byte segment iff one of its bytes exceeds the threshold (strictly, THRESH_TOZERO,
    led_detector.cpp:44) — computed with three SWAR operations per word on the device.  Every threshold from -1 to 255
    (and the clamps beyond) against the byte-wise definition, on segments with one byte at every value around the
    threshold, random segments, all-equal segments; the cheap OR test must never miss a hit."""
    rng = np.random.default_rng(8)
    host.host_scan_tests.restype = C.c_int
    for thr in list(range(-1, 256)) + [-5, 300]:
        t = min(255, max(-1, thr))
        segs = []
        for v in {max(0, t - 1), max(0, t), min(255, t + 1), 0, 127, 128, 255}:
            for pos in (0, 5, 15):
                s = np.full(16, rng.integers(0, max(1, t + 1)) if t >= 0 else 0, np.uint8)  # background <= thr
                s[pos] = v
                segs.append(s)
            segs.append(np.full(16, v, np.uint8))
        segs += [rng.integers(0, 256, 16).astype(np.uint8) for _ in range(20)]
        for s in segs:
            s = np.ascontiguousarray(s)
            want = bool((s.astype(int) > t).any())
            r = host.host_scan_tests(s.ctypes.data_as(C.c_void_p), thr)
            assert bool(r & 1) == want, (thr, s)
            assert (r & 2) or not want, (thr, s)        # maybe_gt16 is a necessary condition
            assert bool(r & 4) == want, (thr, s)        # ... and the compile-time AND / OR forms agree
            assert (r & 8) or not want, (thr, s)


def test_cell_sums_equal_the_border_trace(host):
    """The contour phase without border following (cells_phase: flood per component, Green sums over the 2 x 2 block
    cells of row pairs, Euler-number hole test) against the literal Suzuki-Abe trace (scan_window) on random masks: LED-like
    discs, dense noise with one-pixel-wide bridges and diagonal contacts, rings (holes: the island must go back to the
    trace), several islands side by side and stacked, islands too big for the phase.  Raw contour sums (up to
    orientation), bounding boxes, start keys and the filtered blobs must all agree; the phase must decide most islands
    itself and hand back those with holes."""
    from scipy import ndimage
    host.host_cells_vs_trace.restype = C.c_int
    rng = np.random.default_rng(2024)
    shape_real = np.array([10.0, 200.0, 0.5, 0.5])
    shape_open = np.array([0.0, 1e9, 1.0, 1e9])
    n_comp = n_fb = n_isl = n_hole_isl = 0

    def run(mask, wins, shape):
        nonlocal n_comp, n_fb, n_isl
        mask = np.ascontiguousarray(mask, np.uint8)
        w = np.ascontiguousarray(np.asarray(wins, np.int32).reshape(-1, 4))
        fb = C.c_int(0)
        r = host.host_cells_vs_trace(mask.ctypes.data_as(C.c_void_p), mask.shape[0], mask.shape[1],
                                     w.ctypes.data_as(C.c_void_p), len(w), shape.ctypes.data_as(C.c_void_p), C.byref(fb))
        assert r >= 0, (wins, np.argwhere(mask)[:10])
        n_comp += r
        n_fb += fb.value
        n_isl += len(w)
        return fb.value

    yy, xx = np.mgrid[0:40, 0:120]
    for it in range(1500):
        kind = it % 5
        rows, cols = int(rng.integers(4, 40)), int(rng.integers(4, 120))
        if kind == 0:      # LED-like discs, sometimes touching
            m = np.zeros((rows, cols), bool)
            for _ in range(int(rng.integers(1, 4))):
                cy, cx, rad = rng.uniform(0, rows), rng.uniform(0, cols), rng.uniform(1.0, 6.0)
                m |= (yy[:rows, :cols] - cy) ** 2 + (xx[:rows, :cols] - cx) ** 2 <= rad ** 2
        elif kind == 1:    # dense noise: thin bridges, diagonal contacts, small holes
            m = rng.random((rows, cols)) < rng.uniform(0.2, 0.9)
        elif kind == 2:    # closed noise: blobs with bays
            m = ndimage.binary_closing(rng.random((rows, cols)) < 0.35)
        elif kind == 3:    # a ring (hole) beside a disc
            m = np.zeros((rows, cols), bool)
            cy, cx = rows / 2, cols / 3
            d2 = (yy[:rows, :cols] - cy) ** 2 + (xx[:rows, :cols] - cx) ** 2
            m |= (d2 <= 36) & (d2 >= 9)
            m |= (yy[:rows, :cols] - cy) ** 2 + (xx[:rows, :cols] - 2.2 * cx) ** 2 <= 9
        else:              # sparse specks
            m = rng.random((rows, cols)) < 0.03
        shape = shape_real if it % 2 else shape_open
        run(m, [[0, rows, 0, cols]], shape)
        # the same content as two or three independent islands: column bands with an empty gap, or row bands
        if cols >= 30 and it % 3 == 0:
            c1, c2 = cols // 3, 2 * cols // 3
            m2 = m.copy()
            m2[:, c1 - 1:c1 + 1] = False
            m2[:, c2 - 1:c2 + 1] = False
            run(m2, [[0, rows, 0, c1], [0, rows, c1, c2], [0, rows, c2, cols]], shape)
        if rows >= 12 and it % 3 == 1:
            r1 = rows // 2
            m2 = m.copy()
            m2[r1 - 1:r1 + 1, :] = False
            run(m2, [[0, r1, 0, cols], [r1, rows, 0, cols]], shape)
    # a ring always goes back to the trace; a plain disc never does
    ring = ((yy - 20) ** 2 + (xx - 20) ** 2 <= 64) & ((yy - 20) ** 2 + (xx - 20) ** 2 >= 16)
    assert run(ring[:, :60], [[0, 40, 0, 60]], shape_open) == 1
    disc = (yy - 20) ** 2 + (xx - 20) ** 2 <= 64
    assert run(disc[:, :60], [[0, 40, 0, 60]], shape_open) == 0
    # an island beyond the phase's capacity (rows x words) goes back as a whole
    big = np.zeros((100, 200), bool)
    big[5:90, 10:190] = rng.random((85, 180)) < 0.5
    assert run(big, [[0, 100, 0, 200]], shape_open) == 1
    assert n_comp > 5000 and n_isl > 2000
    assert 0 < n_fb < 0.6 * n_isl, (n_fb, n_isl)


def test_band_scans_equal_the_whole_frame_scan(host):
    """Round 5: the general blob tier (k1b_general) scans one lane per BAND — a maximal run of rows that hold a set
    pixel — instead of one lane over the whole frame.  The decomposition must be exact for findContours(RETR_EXTERNAL):
    same components, raw contour sums, bounding boxes, start keys, filtered blobs.  The device's scan_window (cut out
    of the kernel source) is run over the whole bitmap and then once per band, called as the kernel calls it, on random
    masks: specks of several densities (many short bands, several blobs per band), noise stripes, tall bars through
    many bands' worth of rows, rings with blobs nested inside (not external) and outside, blobs touching the image
    borders, dense noise (one band), widths on both sides of a 64-bit word boundary."""
    from scipy import ndimage
    host.host_bands_vs_whole.restype = C.c_int
    rng = np.random.default_rng(515)
    shape_real = np.array([10.0, 200.0, 0.5, 0.5])
    shape_open = np.array([0.0, 1e9, 1.0, 1e9])
    n_comp = n_bands = n_multi = 0
    for it in range(1200):
        kind = it % 6
        rows = int(rng.integers(3, 70))
        cols = int(rng.choice([rng.integers(3, 60), 61, 62, 63, 64, 65, rng.integers(66, 200)]))
        yy, xx = np.mgrid[0:rows, 0:cols]
        if kind == 0:      # specks: many bands
            m = rng.random((rows, cols)) < rng.choice([0.002, 0.01, 0.03])
            m = ndimage.binary_dilation(m, iterations=int(rng.integers(0, 3))) if rng.random() < 0.7 else m
        elif kind == 1:    # noise stripes separated by empty rows, first / last stripe at the border
            m = np.zeros((rows, cols), bool)
            y = 0
            while y < rows:
                h = int(rng.integers(1, 6))
                m[y:y + h] = rng.random((min(h, rows - y), cols)) < 0.15
                y += h + int(rng.integers(1, 4))
        elif kind == 2:    # a tall bar through the specks
            m = rng.random((rows, cols)) < 0.01
            x0 = int(rng.integers(0, cols))
            m[int(rng.integers(0, rows // 2 + 1)):rows - int(rng.integers(0, rows // 3 + 1)), x0:x0 + 2] = True
        elif kind == 3:    # a ring with blobs inside and outside
            m = rng.random((rows, cols)) < 0.02
            rad = min(rows, cols) / 2.5
            d = np.hypot(yy - rows / 2, xx - cols / 2)
            m |= np.abs(d - rad) < 1.2
        elif kind == 4:    # dense noise: one band, holes, diagonal contacts
            m = rng.random((rows, cols)) < rng.uniform(0.2, 0.7)
        else:              # discs, some cut by the borders
            m = np.zeros((rows, cols), bool)
            for _ in range(int(rng.integers(1, 7))):
                cy, cx, rad = rng.uniform(-2, rows + 2), rng.uniform(-2, cols + 2), rng.uniform(0.8, 6.0)
                m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= rad ** 2
        mask = np.ascontiguousarray(m, np.uint8)
        shape = shape_real if it % 2 else shape_open
        nb = C.c_int(0)
        r = host.host_bands_vs_whole(mask.ctypes.data_as(C.c_void_p), rows, cols, shape.ctypes.data_as(C.c_void_p), C.byref(nb))
        assert r >= 0, (it, kind, rows, cols)
        n_comp += r
        n_bands += nb.value
        n_multi += int(nb.value > 1)
    assert n_comp > 8000 and n_bands > 3000 and n_multi > 500, (n_comp, n_bands, n_multi)
    # the comparison has teeth: a band window that starts one row late must be caught
    os.environ["K1B_HOST_BREAK_BANDS"] = "1"
    try:
        m = np.zeros((20, 30), np.uint8)
        m[3:15, 5:12] = 1
        nb = C.c_int(0)
        assert host.host_bands_vs_whole(m.ctypes.data_as(C.c_void_p), 20, 30, shape_open.ctypes.data_as(C.c_void_p), C.byref(nb)) == -1
    finally:
        del os.environ["K1B_HOST_BREAK_BANDS"]


def test_column_run_scans_equal_the_whole_frame_scan(host):
    """Round 6: the general blob tier cuts every band again at its EMPTY COLUMNS and scans (band, column run) items, one
    lane each (window_column_runs + scan_window<true>, cut out of the kernel source and called as the kernel calls
    them; the runs of a band in reverse order: on the device they run concurrently).  Exact for
    findContours(RETR_EXTERNAL): same components, raw contour sums, bounding boxes, start keys, filtered blobs as the
    whole-frame scan — specks (many runs per band, several sharing a 64-bit word), stripes, bars, rings with blobs
    inside (a ring's columns are one run: what it encloses stays inside it), dense noise, discs cut by the borders,
    widths around the word boundaries."""
    from scipy import ndimage
    host.host_runs_vs_whole.restype = C.c_int
    rng = np.random.default_rng(616)
    shape_real = np.array([10.0, 200.0, 0.5, 0.5])
    shape_open = np.array([0.0, 1e9, 1.0, 1e9])
    n_comp = n_runs = n_multi = 0
    for it in range(1500):
        kind = it % 6
        rows = int(rng.integers(3, 70))
        cols = int(rng.choice([rng.integers(3, 60), 61, 62, 63, 64, 65, 126, 127, 128, 129, rng.integers(66, 400)]))
        if it % 25 == 7:  # bitmap rows of 17 .. 64 words (a wave holds a row's words on 32 / 64 lanes)
            cols = int(rng.choice([957, 958, 959, 1022, 1920, 1983, rng.integers(960, 3900), 3966]))
        yy, xx = np.mgrid[0:rows, 0:cols]
        if kind == 0:
            m = rng.random((rows, cols)) < rng.choice([0.002, 0.01, 0.03])
            m = ndimage.binary_dilation(m, iterations=int(rng.integers(0, 3))) if rng.random() < 0.7 else m
        elif kind == 1:
            m = np.zeros((rows, cols), bool)
            x = 0
            while x < cols:   # noise stripes separated by empty COLUMNS of width 1 .. 3
                w = int(rng.integers(1, 9))
                m[:, x:x + w] = rng.random((rows, min(w, cols - x))) < 0.2
                x += w + int(rng.integers(1, 4))
        elif kind == 2:
            m = rng.random((rows, cols)) < 0.01
            y0 = int(rng.integers(0, rows))
            m[y0:y0 + 2, int(rng.integers(0, cols // 2 + 1)):cols - int(rng.integers(0, cols // 3 + 1))] = True  # a wide bar
        elif kind == 3:
            m = rng.random((rows, cols)) < 0.02
            rad = min(rows, cols) / 2.5
            d = np.hypot(yy - rows / 2, xx - cols / 2)
            m |= np.abs(d - rad) < 1.2
        elif kind == 4:
            m = rng.random((rows, cols)) < rng.uniform(0.05, 0.6)
        else:
            m = np.zeros((rows, cols), bool)
            for _ in range(int(rng.integers(1, 9))):
                cy, cx, rad = rng.uniform(-2, rows + 2), rng.uniform(-2, cols + 2), rng.uniform(0.8, 6.0)
                m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= rad ** 2
        mask = np.ascontiguousarray(m, np.uint8)
        shape = shape_real if it % 2 else shape_open
        nr = C.c_int(0)
        r = host.host_runs_vs_whole(mask.ctypes.data_as(C.c_void_p), rows, cols, shape.ctypes.data_as(C.c_void_p), C.byref(nr))
        assert r >= 0, (it, kind, rows, cols, r)
        n_comp += r
        n_runs += nr.value
        n_multi += int(nr.value > 3)
    assert n_comp > 10000 and n_runs > 8000 and n_multi > 700, (n_comp, n_runs, n_multi)
    os.environ["K1B_HOST_BREAK_RUNS"] = "1"   # the comparison has teeth: a run that starts one column late must be caught
    try:
        m = np.zeros((20, 30), np.uint8)
        m[3:15, 5:12] = 1
        nr = C.c_int(0)
        assert host.host_runs_vs_whole(m.ctypes.data_as(C.c_void_p), 20, 30, shape_open.ctypes.data_as(C.c_void_p), C.byref(nr)) == -1
    finally:
        del os.environ["K1B_HOST_BREAK_RUNS"]


def test_raw_frame_blur_equals_the_blur_of_the_thresholded_copy(host, orc):
    """Round 5: the general blob tier no longer copies the frame; its blur reads the frame's own rows, loads only the
    segments the image pass FLAGGED, applies THRESH_TOZERO on the fly and skips rows without a flagged segment
    (blur_item_fast<.., RAW>).  Against the blur of a thresholded copy (the LDS tiers' input) the non-zero bitmaps must
    be identical: random frames with spots, salt noise, bright patches at the borders (the mirrored-border variant and
    its byte-wise fallback), widths that are not multiples of 16, 3- and 5-tap kernels, thresholds on both sides of
    128, a frame whose first flag bit is not word aligned."""
    host.host_blur_raw_vs_copy.restype = C.c_int
    rng = np.random.default_rng(99)
    total = 0
    for it in range(300):
        rows, cols = int(rng.integers(6, 60)), int(rng.choice([rng.integers(17, 120), 32, 48, 64, 33, 47]))
        img = rng.integers(0, 60, (rows, cols)).astype(np.uint8)
        kind = it % 4
        if kind == 0:
            img[rng.random((rows, cols)) < 0.01] = 255
        elif kind == 1:
            for _ in range(int(rng.integers(1, 5))):
                y, x = int(rng.integers(0, rows)), int(rng.integers(0, cols))
                img[max(0, y - 2):y + 3, max(0, x - 2):x + 3] = rng.integers(100, 256)
        elif kind == 2:   # bright pixels on the borders
            img[:, 0] = rng.integers(0, 256, rows)
            img[:, cols - 1] = rng.integers(0, 256, rows)
            img[0, :] = rng.integers(0, 256, cols)
            img[rows - 1, :] = rng.integers(0, 256, cols)
        else:
            img = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
        thr = int(rng.choice([20, 100, 127, 128, 140, 200, 254]))
        sigma = float(rng.choice([0.4, 0.6, 0.8]))
        taps = np.ascontiguousarray(orc.gaussian_kernel_q8(sigma), np.int32)
        img = np.ascontiguousarray(img)
        r = host.host_blur_raw_vs_copy(img.ctypes.data_as(C.c_void_p), rows, cols, thr, taps.ctypes.data_as(C.c_void_p), len(taps))
        assert r >= 0, (it, rows, cols, thr, sigma)
        total += r
    assert total > 50000


# ---- the shape filter at its edges and every distortion model (detection_parameter_cases.py) ---------------------------

def _same_as_oracle(host, orc, img, kw, K, D, roi_xy, what):
    """host_find_leds against orc.find_leds on the window at roi_xy of a padded image: same count, same order, dist_xy
    and undist_xy equal as bytes."""
    P = orc.make_params(**kw)
    rows, cols = img.shape
    ref_und, ref_dist = orc.find_leds(np.pad(img, ((roi_xy[1], 3), (roi_xy[0], 5))), P, K, D,
                                      roi=(roi_xy[0], roi_xy[1], cols, rows))
    und, dist = _host_find_leds(host, orc, img, P, K, D, roi_xy)
    assert len(dist) == len(ref_dist), (what, len(dist), len(ref_dist))
    assert dist.tobytes() == ref_dist.tobytes() and und.tobytes() == ref_und.tobytes(), what
    return len(dist)


def test_shape_filter_edges_on_the_host(host, orc):
    """The four predicates of blob_filter exactly ON their edges (the statistic itself: kept; the next float64 towards
    rejection: dropped) for every contour of the drawn-shape frame, with the other fields wide open, two mixed points and
    the demo point; a ROI with an odd origin.  The count must also be the one the statistics predict, so a wrong oracle
    and a wrong device source cannot agree by accident."""
    import detection_parameter_cases as dpc
    img = dpc.shape_frame()
    stats = dpc.contour_statistics(orc, img)
    K, D = synth.camera_for(*img.shape)
    pts = dpc.parameter_points(stats)
    assert len(pts) >= 2 * 24
    for label, kw in pts:
        n = _same_as_oracle(host, orc, img, dict(kw, threshold_value=dpc.THR, gaussian_sigma=dpc.SIGMA), K, D, (7, 5), label)
        assert n == dpc.expected_count(stats, kw), (label, n)
    # blobs of width 1 and of height 1: an integer half of 0, the statistic is 0 / 0 and never <= anything
    thin = dpc.thin_frame()
    tstats = dpc.contour_statistics(orc, thin, sigma=0.2)
    for mc in (1e9, float("inf")):
        kw = dict(dpc.OPEN, max_circular_distortion=mc)
        n = _same_as_oracle(host, orc, thin, dict(kw, threshold_value=dpc.THR, gaussian_sigma=0.2), K, D, (3, 1), ("thin", mc))
        assert n == dpc.expected_count(tstats, kw) == 1, (mc, n)


def test_both_contour_phases_see_the_filter_edges(host, orc):
    """cells_phase (the cell sums; island_record) and scan_window (the literal trace) on the drawn-shape mask, one island
    window per shape, at a handful of edge points: the kept blobs agree, the ring (a hole) is the one island handed back
    to the trace, the seven others are decided by the cell sums."""
    from scipy import ndimage
    import detection_parameter_cases as dpc
    host.host_cells_vs_trace.restype = C.c_int
    img = dpc.shape_frame()
    stats = dpc.contour_statistics(orc, img)
    _, mask = orc.blur_mask(img, dpc.THR, dpc.SIGMA)
    mask = np.ascontiguousarray(mask > 0, np.uint8)
    lab, n = ndimage.label(mask, structure=np.ones((3, 3), int))
    wins = np.ascontiguousarray([[s[0].start, s[0].stop, s[1].start, s[1].stop] for s in ndimage.find_objects(lab)], np.int32)
    assert n == len(stats) == 8
    pts = dpc.parameter_points(stats)
    pick = [p for p in pts if "@76.0" in p[0] or "0.5333" in p[0] or "1.6879" in p[0] or "0.5048" in p[0] or p[0] == "demo"]
    assert len(pick) >= 9
    for label, kw in pick:
        shape = np.array([kw[f] for f in dpc.FIELDS])
        fb = C.c_int(0)
        r = host.host_cells_vs_trace(mask.ctypes.data_as(C.c_void_p), mask.shape[0], mask.shape[1],
                                     wins.ctypes.data_as(C.c_void_p), len(wins), shape.ctypes.data_as(C.c_void_p), C.byref(fb))
        assert r == 8 and fb.value == 1, (label, r, fb.value)


def test_distortion_models_on_the_host(host, orc):
    """undistort_point with 0, 4, 5, 8 and 12 coefficients and a skewed K (detection_parameter_cases.CAMERAS) against the
    oracle on frames of spots, wide-open and demo filter, with and without a ROI origin."""
    import detection_parameter_cases as dpc
    n_blobs = 0
    for c, (name, (K, D)) in enumerate(dpc.CAMERAS.items()):
        rng = np.random.default_rng(40 + c)
        for it in range(4):
            img = dpc.spots_frame(rng, K, D)
            kw = dict(dpc.OPEN) if it % 2 else {}
            n_blobs += _same_as_oracle(host, orc, img, kw, K, D, (11, 3) if it < 2 else (0, 0), (name, it))
    assert n_blobs >= 7 * 4 * 6, n_blobs


# ---- frames at the frame-size capacity, 4096 x 4000 (frame_size_cases.py) -------------------------------------------------
# What this tier reaches of the capacity: the literal whole-frame scan (host_find_leds: scan_window over all rows by one
# lane, which IS k1b_general's fallback for more than 768 bands), the band and (band, column run) decompositions with
# bitmap rows of 64 words and 4 096 rows, and lds_set_range on all 64 words of the row bitset.  What it does not reach,
# because it is wave code that could only be restated here, not compiled: the lanes-per-row grouping (lw = 6) of
# k1b_general's column occupancy, its band list (prefix sums over 64 lanes, the 768-entry cap), the front phase's band
# builder and its s_colocc words.  Those are the GPU tier's (tests/test_frame_size_capacity.py).

def _touch_bands(mask):
    """k1b_general's bands, in numpy: maximal runs of non-empty rows in which every row has a pixel 8-adjacent to one of
    the row above."""
    m = np.asarray(mask, bool)
    act = m.any(axis=1)
    up = np.zeros_like(m)
    up[1:] = m[:-1]
    near = up.copy()
    near[:, 1:] |= up[:, :-1]
    near[:, :-1] |= up[:, 1:]
    linked = (m & near).any(axis=1)
    return int((act & ~linked).sum())


def test_capacity_geometry_is_what_the_shapes_are_named_for():
    """wb, lw, rw and the pitch of every shape of frame_size_cases.py from make_geom's formulas, and the budget
    arithmetic the refusal tests rely on — numbers only, no device code."""
    import frame_size_cases as fsc
    g = {s: fsc.geom(*s) for s in fsc.NARROW + [fsc.FULL]}
    assert g[17, 4000]["wb"] == 64 and g[17, 4000]["lw"] == 6 and g[17, 4000]["pitch"] == 4000
    assert g[17, 3999]["wb"] == 64 and g[17, 3999]["pitch"] == 4000 != 3999
    assert g[17, 3967]["wb"] == 64 and g[17, 3966]["wb"] == 63
    assert (g[17, 1983]["wb"], g[17, 1983]["lw"]) == (33, 6) and (g[17, 1982]["wb"], g[17, 1982]["lw"]) == (32, 5)
    assert g[4096, 33]["rw"] == 64 and g[4095, 33]["rw"] == 64 and g[4096, 33]["pitch"] == 48
    assert g[1537, 33]["rw"] == 25 and g[1600, 48]["pitch"] == 48
    assert g[fsc.FULL]["wb"] == 64 and g[fsc.FULL]["rw"] == 64 and g[fsc.FULL]["segs_per_row"] == 250
    # no frame make_geom accepts has a bitmap row of more than 64 words (the g.wb > 64 branch of k1b_general)
    assert max(fsc.geom(1, c)["wb"] for c in range(1, fsc.MAX_COLS + 1)) == 64 and fsc.geom(1, 4031)["wb"] == 65
    assert fsc.slot_cap(17, 4000, 8192) == 5 < 8 <= fsc.slot_cap(17, 752, 8192) and fsc.slot_cap(17, 4000) >= 8
    assert fsc.slot_cap(*fsc.FULL) >= 8


def test_capacity_frames_hold_what_the_tests_need(orc):
    """The requirements on the drawn frames, against the oracle's blurred mask and detections, so that a later edit cannot
    empty the tests: spots whose mask touches the last row and the last column, masks across x = 1023/1024, 2047/2048,
    3071/3072 and y = 63/64, 4031/4032, detections on the far side of each, at most 64 of them with and without the
    salt, and the salt only in the far quarter."""
    import frame_size_cases as fsc
    for rows, cols in fsc.NARROW:
        K, D = synth.camera_for(rows, cols)
        plain, salted = fsc.frame(rows, cols), fsc.frame(rows, cols, True)
        _, mask = orc.blur_mask(plain["img"], 140, 0.6)
        mask = mask > 0
        assert mask[rows - 1].any() and mask[:, cols - 1].any() and mask[rows - 1, cols - 1], (rows, cols)
        for x in (1024, 2048, 3072):
            if x + 25 < cols:
                assert (mask[:, x - 1] & mask[:, x]).any(), (rows, cols, x)
        for y in (64, 4032):
            if y + 9 < rows:
                assert (mask[y - 1] & mask[y]).any(), (rows, cols, y)
        und, dist = orc.find_leds(plain["img"], orc.make_params(), K, D)
        und_s, dist_s = orc.find_leds(salted["img"], orc.make_params(), K, D)
        assert 4 <= len(dist) <= 64 and dist_s.tobytes() == dist.tobytes(), (rows, cols, len(dist), len(dist_s))
        assert dist[:, 0].max() > cols - 8 and dist[:, 1].max() > rows - 8, (rows, cols)
        diff = np.argwhere(plain["img"] != salted["img"])
        assert len(diff) == salted["n_salt"] > 30 and diff[:, 0].min() >= rows / 2 and diff[:, 1].min() >= cols / 2


def test_capacity_shapes_on_the_host(host, orc):
    """The device blob source over every narrow shape, plain and with the far-quarter salt: the oracle's detections,
    byte for byte; one shape again behind a ROI origin beyond (2048, 1200)."""
    import frame_size_cases as fsc
    n = 0
    for rows, cols in fsc.NARROW:
        K, D = synth.camera_for(rows, cols)
        for clutter in (False, True):
            n += _same_as_oracle(host, orc, fsc.frame(rows, cols, clutter)["img"], {}, K, D, (0, 0), (rows, cols, clutter))
    K, D = synth.camera_for(1300, 4100)
    n += _same_as_oracle(host, orc, fsc.frame(17, 1983, True)["img"], {}, K, D, (2051, 1203), "origin")
    assert n >= 21 * 5, n
    # windows of 1, 2 and 3 rows (the last rows of a strip, a one-column window of a column shape): the blur mirrors a
    # one-row window onto itself; with the filter wide open every contour counts
    kw = dict(min_blob_area=0.0, max_blob_area=1e9, max_width_height_distortion=1e9, max_circular_distortion=1e9)
    m = 0
    for img in (fsc.frame(17, 4000, True)["img"], fsc.frame(17, 1982)["img"]):
        K, D = synth.camera_for(*img.shape)
        for h in (1, 2, 3):
            m += _same_as_oracle(host, orc, np.ascontiguousarray(img[17 - h:]), {}, K, D, (0, 17 - h), h)
            P = orc.make_params(**kw)
            ref_und, ref_dist = orc.find_leds(img, P, K, D, roi=(0, 17 - h, img.shape[1], h))
            und, dist = _host_find_leds(host, orc, np.ascontiguousarray(img[17 - h:]), P, K, D, (0, 17 - h))
            assert np.array_equal(dist, ref_dist, equal_nan=True) and np.array_equal(und, ref_und, equal_nan=True), h
            m += len(dist)
    col = fsc.frame(4096, 33)["img"]
    m += _same_as_oracle(host, orc, np.ascontiguousarray(col[:, 32:]), kw, *synth.camera_for(4096, 33), (32, 0), "column")
    assert m >= 20, m


def test_capacity_row_bitset_on_the_host(host):
    """lds_set_range, as the front phase calls it for every bright segment (rows y - r .. y + r, clipped), on frames of
    4 096 and 4 095 rows: the 64 words against numpy's dilation of the rows that hold a pixel above the threshold; words
    32 .. 63 (the 1 200-row frames of the other tests end in word 18) all hold a bit."""
    import frame_size_cases as fsc
    for rows, cols in ((4096, 33), (4095, 33), (17, 4000)):
        for r in (1, 2, 4):
            img = fsc.frame(rows, cols, True)["img"]
            ys = np.nonzero((img > 140).any(axis=1))[0]
            lohi = np.ascontiguousarray(np.stack([np.maximum(0, ys - r), np.minimum(rows - 1, ys + r)], 1), np.int32)
            bits = np.zeros(64, np.uint64)
            host.host_set_row_ranges(bits.ctypes.data_as(C.c_void_p), lohi.ctypes.data_as(C.c_void_p), len(lohi))
            want = np.zeros(4096, bool)
            for lo, hi in lohi:
                want[lo:hi + 1] = True
            got = np.unpackbits(bits.view(np.uint8), bitorder="little").astype(bool)
            assert np.array_equal(got, want), (rows, cols, r)
            if rows >= 4095:
                assert bits[32:].all(), (rows, r)     # the salt: a bit in every word of the rows from 2 048 on
                assert got[rows - 1] and not got[rows:].any()


def test_capacity_bands_and_column_runs_on_the_host(host, orc):
    """scan_window per band and per (band, column run) — the decompositions of k1b_general, called as the kernel calls
    them — against the whole-frame scan on the blurred masks of 17 x 4000 (bitmap rows of 64 words: the kernel's limit),
    17 x 3999, 4096 x 33 and 4095 x 33, plain, salted, and the band frames; the band count is numpy's."""
    import frame_size_cases as fsc
    host.host_bands_vs_whole.restype = C.c_int
    host.host_runs_vs_whole.restype = C.c_int
    shape = np.array([10.0, 200.0, 0.5, 0.5])
    cases = [(fsc.frame(r, c, s)["img"], 0.6, 0) for r, c in ((17, 4000), (17, 3999), (4096, 33), (4095, 33)) for s in (False, True)]
    for r, c, sigma, ns in ((4096, 33, fsc.BAND_SIGMA, 6), (4095, 33, fsc.BAND_SIGMA, 6), (1537, 33, fsc.TIGHT_SIGMA, 0),
                            (1600, 48, fsc.TIGHT_SIGMA, 2), (1536, 33, fsc.TIGHT_SIGMA, 0)):
        b = fsc.band_frame(r, c, sigma, ns)
        cases.append((b["img"], sigma, b["n_bands"]))
    for img, sigma, at_least in cases:
        rows, cols = img.shape
        _, mask = orc.blur_mask(img, 140, sigma)
        mask = np.ascontiguousarray(mask > 0, np.uint8)
        want = _touch_bands(mask)
        assert want >= fsc.count_bands(mask) >= at_least, (rows, cols, want, at_least)
        nb, nr = C.c_int(0), C.c_int(0)
        rb = host.host_bands_vs_whole(mask.ctypes.data_as(C.c_void_p), rows, cols, shape.ctypes.data_as(C.c_void_p), C.byref(nb))
        rr = host.host_runs_vs_whole(mask.ctypes.data_as(C.c_void_p), rows, cols, shape.ctypes.data_as(C.c_void_p), C.byref(nr))
        assert rb >= 1 and rr == rb and nb.value == want and nr.value >= want, (rows, cols, sigma, rb, rr, nb.value, nr.value, want)


def test_band_frames_guarantee_their_band_count(host, orc):
    """The band frames: more than 768 bands (K1B_GEN_BANDS: the whole-frame fallback of k1b_general) on 4096 x 33,
    4095 x 33 (sigma 0.3, a lone pixel every 4 rows) and on 1537 x 33, 1600 x 48 (sigma 0.2, every 2 rows: no frame of
    fewer rows can hold that many), exactly 768 on the 1536-row control — counted from how the frame was drawn and
    confirmed on the oracle's mask; the oracle drops every lone pixel and keeps the spots; the device source's
    whole-frame scan gives the oracle's bytes."""
    import frame_size_cases as fsc
    for rows, cols, sigma, ns, over in ((4096, 33, fsc.BAND_SIGMA, 6, True), (4095, 33, fsc.BAND_SIGMA, 6, True),
                                        (1537, 33, fsc.TIGHT_SIGMA, 0, True), (1600, 48, fsc.TIGHT_SIGMA, 2, True),
                                        (1536, 33, fsc.TIGHT_SIGMA, 0, False), (1536, 33, fsc.BAND_SIGMA, 6, False)):
        b = fsc.band_frame(rows, cols, sigma, ns)
        _, mask = orc.blur_mask(b["img"], 140, sigma)
        n_mask = fsc.count_bands(mask > 0)
        assert (b["n_bands"] > fsc.GEN_BANDS) == over and n_mask >= b["n_bands"], (rows, cols, sigma, b["n_bands"], n_mask)
        assert over or n_mask <= fsc.GEN_BANDS, (rows, n_mask)
        K, D = synth.camera_for(rows, cols)
        n = _same_as_oracle(host, orc, b["img"], dict(gaussian_sigma=sigma), K, D, (0, 0), (rows, cols, sigma))
        assert n == ns, (rows, cols, sigma, n)
