"""Inputs shared by the shape-filter and distortion-model tests (test_detection_parameters.py, test_k1b_host.py):
a frame of drawn shapes whose four filter statistics are computed here, in float64 and in the reference's order of
operations (led_detector.cpp:65-86), the parameter points that sit exactly on every predicate's edge, and cameras with
4, 5, 8 and 12 distortion coefficients.  Nothing here touches the device code or the oracle's filter: the oracle only
supplies the blurred mask and its external contours."""
import numpy as np

from rpg_monocular_pose_estimator_amd import synth

THR, SIGMA = 140, 0.6
ROWS, COLS = 64, 160
FIELDS = ("min_blob_area", "max_blob_area", "max_width_height_distortion", "max_circular_distortion")
OPEN = dict(min_blob_area=0.0, max_blob_area=1e9, max_width_height_distortion=1e9, max_circular_distortion=1e9)


def shape_frame():
    """Eight drawn shapes on black, far enough apart that their blurred masks stay separate."""
    f = np.zeros((ROWS, COLS), np.uint8)
    f[6:10, 6:10] = 255                        # 4 x 4 square
    f[8:11, 20:31] = 255                       # 11 x 3 bar (wide)
    f[5:16, 42:45] = 255                       # 3 x 11 bar (tall)
    yy, xx = np.mgrid[0:ROWS, 0:COLS]
    f[(yy - 12) ** 2 + (xx - 64) ** 2 <= 36] = 255                              # disc of radius 6
    f[((yy - 10) / 2.0) ** 2 + ((xx - 90) / 4.5) ** 2 <= 1.0] = 255             # 9 x 4 ellipse
    f[30:42, 8:20] = 255                       # 12 x 12 square ring ...
    f[33:39, 11:17] = 0                        # ... with a 6 x 6 hole
    f[36, 40] = 255                            # a single pixel
    f[30:35, 60:65] = 255                      # two 5 x 5 squares ...
    f[35:40, 65:70] = 255                      # ... touching at a corner
    return f


def thin_frame():
    """For sigma 0.2 (taps [0, 256, 0]: the mask is the thresholded frame itself): blobs of width 1, of height 1, a
    single pixel (both) and one ordinary square."""
    f = np.zeros((32, 64), np.uint8)
    f[4:11, 5] = 255         # 1 x 7
    f[6, 12:21] = 255        # 9 x 1
    f[16, 30] = 255          # 1 x 1
    f[20:25, 40:45] = 255    # 5 x 5
    return f


def contour_statistics(orc, img, thr=THR, sigma=SIGMA):
    """The statistics the four predicates compare, per external contour of the blurred mask, in findLeds' order (newest
    contour first is the order of its output; here the order is external_contours').  -> list of dicts."""
    from scipy import ndimage
    _, mask = orc.blur_mask(img, thr, sigma)
    lab, _ = ndimage.label(mask > 0, structure=np.ones((3, 3), int))
    out = []
    for c in orc.external_contours(mask):
        x, y = c[:, 0].astype(np.float64), c[:, 1].astype(np.float64)
        xp, yp = np.roll(x, 1), np.roll(y, 1)
        area = np.float64(abs(float((xp * y - yp * x).sum()) * 0.5))          # cv::contourArea
        w = int(c[:, 0].max() - c[:, 0].min() + 1)
        h = int(c[:, 1].max() - c[:, 1].min() + 1)
        with np.errstate(all="ignore"):
            wh = np.abs(1 - min(np.float64(w) / np.float64(h), np.float64(h) / np.float64(w)))
            cw = np.abs(1 - area / (np.float64(np.pi) * np.float64((w // 2) ** 2)))   # INTEGER halves
            ch = np.abs(1 - area / (np.float64(np.pi) * np.float64((h // 2) ** 2)))
        comp = lab == lab[c[0, 1], c[0, 0]]
        out.append(dict(area=area, wh=wh, circ_w=cw, circ_h=ch, w=w, h=h,
                        # both circular tests must hold: the larger statistic decides (a NaN never passes)
                        circ=np.float64(np.nan) if np.isnan(cw) or np.isnan(ch) else max(cw, ch),
                        hole=bool((ndimage.binary_fill_holes(comp) & ~comp).any())))
    return out


def expected_count(stats, P):
    """How many contours the four predicates keep, from the statistics alone."""
    n = 0
    for s in stats:
        with np.errstate(all="ignore"):
            n += bool(s["area"] >= P["min_blob_area"] and s["area"] <= P["max_blob_area"] and
                      s["wh"] <= P["max_width_height_distortion"] and s["circ_w"] <= P["max_circular_distortion"] and
                      s["circ_h"] <= P["max_circular_distortion"])
    return n


def edge_points(stats):
    """For every contour and every predicate: the parameter value at which the contour is still kept (its own statistic:
    every comparison is inclusive), the next float64 towards rejection, and how many contours share the statistic.
    The other three fields are wide open.  -> list of (label, field, keep value, drop value, n sharing), one entry per
    distinct (field, statistic)."""
    key = dict(min_blob_area="area", max_blob_area="area", max_width_height_distortion="wh", max_circular_distortion="circ")
    pts = []
    for field in FIELDS:
        vals = [s[key[field]] for s in stats]
        for v in sorted(set(float(v) for v in vals if np.isfinite(v))):
            drop = np.nextafter(v, np.inf if field == "min_blob_area" else -np.inf)
            pts.append(("%s@%r" % (field, v), field, float(v), float(drop), sum(1 for u in vals if float(u) == v)))
    return pts


def parameter_points(stats):
    """Every parameter point of the edge table as a dict of the four filter fields (keep and drop of every edge), then a
    few mixed points where two fields bind at once."""
    out = []
    for label, field, keep, drop, _ in edge_points(stats):
        out.append((label + ":keep", dict(OPEN, **{field: keep})))
        out.append((label + ":drop", dict(OPEN, **{field: drop})))
    areas = sorted(set(float(s["area"]) for s in stats))
    circ = sorted(set(float(s["circ"]) for s in stats if np.isfinite(s["circ"])))
    out.append(("mixed:area-window", dict(OPEN, min_blob_area=areas[1], max_blob_area=areas[-2])))
    out.append(("mixed:circ+wh", dict(OPEN, max_circular_distortion=circ[len(circ) // 2], max_width_height_distortion=0.5)))
    out.append(("demo", dict(min_blob_area=10.0, max_blob_area=200.0, max_width_height_distortion=0.5,
                             max_circular_distortion=0.5)))
    return out


# ---- cameras ---------------------------------------------------------------------------------------------------------
D4 = synth.README_D[:4].copy()
D5 = synth.README_D.copy()
D5[4] = -0.035
D8 = np.array([0.35, -0.12, 5e-4, -2e-4, 0.02, 0.72, -0.05, 0.004])
D12 = np.concatenate([D8, [0.01, -0.02, 0.03, -0.04]])
K_SKEW = synth.README_K.copy()
K_SKEW[0, 1] = 0.8
CAMERAS = {"D0": (synth.README_K, np.zeros(0)), "README": (synth.README_K, synth.README_D), "D4": (synth.README_K, D4),
           "D5": (synth.README_K, D5), "D8": (synth.README_K, D8), "D12": (synth.README_K, D12),
           "K_skew": (K_SKEW, D8)}


def forward_rational(xy, K, D):
    """Pinhole pixel -> distorted pixel through OpenCV's documented rational model (k1 k2 p1 p2 k3 k4 k5 k6; missing
    coefficients are zero), plain float64.  Written from the model's definition, not from any inverse."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    k1, k2, p1, p2, k3, k4, k5, k6 = (list(np.asarray(D, np.float64).reshape(-1)[:8]) + [0.0] * 8)[:8]
    xy = np.asarray(xy, np.float64)
    y = (xy[..., 1] - K[1, 2]) / K[1, 1]
    x = (xy[..., 0] - K[0, 2] - K[0, 1] * y) / K[0, 0]
    r2 = x * x + y * y
    rad = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([K[0, 0] * xd + K[0, 1] * yd + K[0, 2], K[1, 1] * yd + K[1, 2]], -1)


def spots_frame(rng, K, D, rows=120, cols=200, n=9):
    """Gaussian spots spread over a small frame (detection entries only: K is used as it stands, so the points lie far
    from the principal point and the distortion terms are large)."""
    spots = np.stack([rng.uniform(8, cols - 8, n), rng.uniform(8, rows - 8, n)], 1)
    return synth.render_frame(rng, spots, rows, cols)


# ---- scenes rendered through the forward rational model --------------------------------------------------------------

def _in_view(px, rows, cols, margin):
    d = np.linalg.norm(px[:, None, :] - px[None, :, :], axis=-1) + np.eye(len(px)) * 1e9
    return (px[:, 0].min() >= margin and px[:, 0].max() <= cols - 1 - margin and px[:, 1].min() >= margin and
            px[:, 1].max() <= rows - 1 - margin and d.min() >= 12.0)


def _pose(rng, lateral, depth):
    T = np.eye(4)
    T[:3, :3] = synth.rodrigues(rng.normal(size=3), rng.uniform(0.0, 0.8))
    T[:3, 3] = [rng.uniform(-lateral[0], lateral[0]), rng.uniform(-lateral[1], lateral[1]), rng.uniform(*depth)]
    return T


def rational_sequence(n, seed, cameras, T_cam_rig=None, markers=synth.M5, rows=480, cols=752, lateral=(0.1, 0.08),
                      depth=(1.0, 1.8), margin=100.0, dt=0.02, lin_speed=0.15, ang_speed=0.6):
    """synth.make_rig_sequence's trajectory model (constant twist + small jitter, frame k at k * dt) for a body seen by
    cameras [(K, D)] with extrinsics T_cam_rig (camera <- rig; default: one camera, the identity), every LED rendered at
    its forward_rational position.  lateral / depth bound the first pose's translation (the defaults keep the body near
    the image centre, where the reference's polynomial-only ROI placement still finds it); margin: pixels every LED keeps
    from the image border in every camera.  -> dict(frames [N arrays (n, rows, cols)], T_true (n, 4, 4), T_true_cam,
    times, markers)."""
    E = np.eye(4)[None] if T_cam_rig is None else np.asarray(T_cam_rig, np.float64).reshape(-1, 4, 4)
    M = np.asarray(markers, np.float64)
    rng = np.random.default_rng([seed, 23])
    E0_inv = np.linalg.inv(E[0])
    for _ in range(20000):
        T0 = E0_inv @ _pose(rng, lateral, depth)
        v = rng.normal(size=3)
        v *= lin_speed / np.linalg.norm(v)
        w = rng.normal(size=3)
        w *= ang_speed / np.linalg.norm(w)
        Ts = []
        for k in range(n):
            Tk = np.eye(4)
            Tk[:3, :3] = synth.rodrigues(w, np.linalg.norm(w) * k * dt) @ T0[:3, :3]
            Tk[:3, 3] = T0[:3, 3] + v * k * dt + 0.0005 * rng.normal(size=3)
            if not all((Ec @ Tk)[2, 3] >= 0.5 and _in_view(forward_rational(synth.project(Ec @ Tk, M, K), K, D), rows, cols, margin)
                       for (K, D), Ec in zip(cameras, E)):
                break
            Ts.append(Tk)
        if len(Ts) == n:
            break
    else:
        raise ValueError("rational_sequence: no trajectory stays in view")
    frames = []
    for c, ((K, D), Ec) in enumerate(zip(cameras, E)):
        fr = np.empty((n, rows, cols), np.uint8)
        for k in range(n):
            px = forward_rational(synth.project(Ec @ Ts[k], M, K), K, D)
            fr[k] = synth.render_frame(np.random.default_rng([seed, k, 3, c]), px, rows, cols, 1.5)
        frames.append(fr)
    return dict(frames=frames, T_true=np.array(Ts), T_true_cam=np.array([[Ec @ T for T in Ts] for Ec in E]),
                times=np.arange(n) * dt, markers=M, rows=rows, cols=cols)


def rational_frames(n, seed, K, D, **kw):
    """n independent frames (sequences of one frame each, rational_sequence's keywords) -> (frames (n, rows, cols), T_true)."""
    seqs = [rational_sequence(1, 1000 * seed + i, [(K, D)], **kw) for i in range(n)]
    return np.stack([q["frames"][0][0] for q in seqs]), np.stack([q["T_true"][0] for q in seqs])


def cluttered_shape_frames(n, seed, rows=300, cols=176, first=72, step=6):
    """The drawn shapes (at an odd offset) above a column of single bright pixels, one every `step` rows: each is a band
    of its own, and 38 bands are more than either LDS tier of the blob kernel takes (8 and 32), so the frame goes to the
    general tier.  8 + 38 contours, fewer than MPE_MAX_DETECTIONS."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, rows, cols), np.uint8)
    for f in out:
        f[5:5 + ROWS, 7:7 + COLS] = shape_frame()
        for y in range(first, rows - 3, step):
            f[y, int(rng.integers(3, cols - 3))] = 255
    return out
