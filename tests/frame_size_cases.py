"""Inputs shared by the frame-size capacity tests (test_frame_size_capacity.py, test_k1b_host.py): frames at and just
below the largest size the library takes (make_geom, csrc/mpe_schedule.cpp: rows <= 4096, cols <= 4000), each shape the
smallest that still reaches the structure it is named for, with Gaussian spots (synth.render_frame, drawn into patches)
on the word boundaries of the blob kernels' bitsets and on the frame's last row and column.  The geometry every test
asserts (wb, lw, rw, pitch) is computed HERE from the frame size with make_geom's formulas, never read back from the
library.  Plain numpy: nothing here touches the device code or the oracle."""
import numpy as np

from rpg_monocular_pose_estimator_amd import synth

MAX_ROWS, MAX_COLS = 4096, 4000      # make_geom's cap: s_rowact[64] holds a bit per row, a bitmap row at most 64 words
FULL = (MAX_ROWS, MAX_COLS)
GEN_BANDS = 768                      # K1B_GEN_BANDS (csrc/mpe_k1.hip): more bands and one lane scans the whole frame
# (rows, cols): why
SHAPES = {
    (17, 4000): "wb 64, colocc words 0..3, pitch == cols: the packed path, no repack",
    (17, 3999): "pitch 4000 != cols: the repack path",
    (17, 3967): "wb 64, the last width with it",
    (17, 3966): "wb 63",
    (17, 1983): "wb 33: lw 6, the first width with it",
    (17, 1982): "wb 32: lw 5",
    (4096, 33): "rowact words up to 63, odd pitch",
    (4095, 33): "the last row is bit 62 of word 63",
    (1537, 33): "one row past the 1 536 of the band list",
    (1600, 48): "rows past 1 536, pitch == cols",
}
NARROW = list(SHAPES)
BAND_SIGMA = 0.3                     # taps [1, 254, 1]: a lone 255 pixel lights its four edge neighbours, support +-1
TIGHT_SIGMA = 0.2                    # taps [0, 256, 0]: the mask is the thresholded frame, support +-0


def geom(rows, cols):
    """make_geom's arithmetic (csrc/mpe_schedule.cpp) and k1b_general's choice of lanes per bitmap row (csrc/mpe_k1.hip),
    restated: pitch (row of 16-byte segments), wb (64-bit words of a bitmap row: a pad column either side, a pad word),
    rw (words of the row bitset), tw (words of a row's segment bits), lw (log2 of the lanes that share a bitmap row)."""
    pitch = (cols + 15) & ~15
    wb = (cols + 2 + 63) // 64 + 1
    return dict(pitch=pitch, segs_per_row=pitch // 16, wb=wb, rw=(rows + 63) // 64, tw=(pitch // 16 + 63) // 64,
                lw=4 if wb <= 16 else (5 if wb <= 32 else 6))


def slot_cap(rows, cols, lds_budget=64 * 1024):
    """make_geom's budget question: the bitmap rows of this width that `lds_budget` bytes hold; below 8 the frame is
    refused, whatever its height."""
    g = geom(rows, cols)
    per_slot = (3 * g["wb"] + g["tw"]) * 8 + g["wb"] // 8 + 1
    fixed = 2 * g["rw"] * 8 + 2 * g["rw"] * 4 + 64
    return (lds_budget - fixed) // per_slot


def spot_centres(rows, cols):
    """Where the spots go, as (x, y): the four corners (3 px in: the blurred mask of a sigma-1.5 spot is 4 px in radius,
    so it is cut by the last row and the last column), the last row, the boundaries of 64-bit words of the column
    occupancy (x = 2047/2048, 3071/3072; 1023/1024) and of the row bitset (y = 63/64, 4031/4032), and spots at least 5 px
    from every edge.  Only what fits the frame; every pair at least 14 px apart in x or in y."""
    c = [(3.0, 3.0), (cols - 4.0, 3.0), (3.0, rows - 4.0), (cols - 4.0, rows - 4.0)]
    ys = [y for y in (63.5, 4031.5, rows / 2.0 + 0.25) if 8 <= y <= rows - 9] or [rows / 2.0]
    xs = [x for x in (1023.5, 2047.5, 3071.5, cols / 2.0 + 0.3) if 24 <= x <= cols - 25] or [cols / 2.0]
    if rows <= 64:        # a strip: spots along x, in the middle rows and on the last row
        for k, x in enumerate(xs):
            c.append((x, ys[0] + 0.2 * k))
            c.append((x + 17.0, rows - 1.0))
    elif cols <= 64:      # a column: spots along y, in the middle columns
        for k, y in enumerate(ys):
            c.append((cols / 2.0 + 0.2 * k, y))
        c.append((cols / 2.0, rows - 1.0))
    else:                 # both axes: every word boundary of x on every word boundary of y, and on the last row
        for y in ys:
            for x in xs:
                c.append((x, y))
        for x in xs:
            c.append((x + 17.0, rows - 1.0))
        c.append((cols - 4.0, 2047.5))                     # the last column, half way down
    return np.array(c, np.float64)


def _paste_spots(f, spots, seed, sigma=1.5):
    """The spots of synth.render_frame, each drawn into a patch of its own (noise of the patch included) and pasted."""
    rows, cols = f.shape
    rad = int(np.ceil(4 * sigma)) + 1
    for k, (sx, sy) in enumerate(spots):
        x0, x1 = max(0, int(np.floor(sx)) - rad), min(cols, int(np.floor(sx)) + rad + 2)
        y0, y1 = max(0, int(np.floor(sy)) - rad), min(rows, int(np.floor(sy)) + rad + 2)
        patch = synth.render_frame(np.random.default_rng([seed, k, 5]), [(sx - x0, sy - y0)], y1 - y0, x1 - x0, sigma)
        f[y0:y1, x0:x1] = np.maximum(f[y0:y1, x0:x1], patch)
    return f


def _background(rng, rows, cols):
    return rng.integers(0, 30, (rows, cols), dtype=np.uint8)


def salt_far_quarter(f, spots, seed):
    """Salt confined to the far quarter (x >= cols / 2, y >= rows / 2): every fourth row, one pixel in every 16-pixel
    segment at a random place inside it (2 .. 13: neighbours at least 5 columns apart), value 150 .. 190.  Under the demo
    parameters (threshold 140, taps [1, 42, 170, 42, 1]) such a pixel's blurred mask is its 3 x 3 neighbourhood (190 * 170
    < 2^15 keeps the taps of weight 1 out), so no two masks touch and each is a contour of area 4 that min_blob_area
    drops: the detections stay those of the spots.  Every segment column of the quarter is occupied in every band of
    rows, which makes one island wider or taller than the LDS tiers' pixel pools (12 288 bytes), or more bright segments
    than their lists hold (512): the frame goes to the general tier.  Pixels within 12 px of a spot are left out.
    -> number of salt pixels."""
    rows, cols = f.shape
    rng = np.random.default_rng([seed, 29])
    n = 0
    for y in range((rows + 1) // 2, rows, 4):
        for x0 in range((cols // 2 + 15) & ~15, cols - 15, 16):
            x = x0 + int(rng.integers(2, 14))
            if np.all(np.maximum(np.abs(spots[:, 0] - x), np.abs(spots[:, 1] - y)) > 12):
                f[y, x] = int(rng.integers(150, 191))
                n += 1
    return n


_FRAMES = {}


def frame(rows, cols, clutter=False, seed=0):
    """-> dict(img (rows, cols) uint8 — shared, do not write to it —, spots (n, 2), n_salt)."""
    key = (rows, cols, bool(clutter), seed)
    if key not in _FRAMES:
        spots = spot_centres(rows, cols)
        f = _paste_spots(_background(np.random.default_rng([seed, rows, cols]), rows, cols), spots, seed)
        n_salt = salt_far_quarter(f, spots, seed) if clutter else 0
        f.setflags(write=False)
        _FRAMES[key] = dict(img=f, spots=spots, n_salt=n_salt)
    return _FRAMES[key]


def band_frame(rows, cols, sigma=BAND_SIGMA, n_spots=6, seed=0):
    """Lone 255 pixels, one every `step` rows at a varying x, on a dim background, and n_spots real spots.  sigma 0.3
    (ksize 3, r = 1): a pixel's mask covers rows y - 1 .. y + 1, step 2r + 2 = 4 leaves an empty row between neighbours;
    sigma 0.2 (taps [0, 256, 0]): the mask is the pixel, step 2.  So every lone pixel is a band of its own — a maximal
    run of non-empty rows of the blurred mask — by construction, and n_bands (the lone pixels drawn; those within 8 rows
    of a spot are left out, and the spots' own bands are not counted) is a LOWER bound of the frame's band count that
    owes nothing to the code under test.  The shape filter drops a lone pixel (sigma 0.3: a plus of contour area 2;
    sigma 0.2: width 1).  -> dict(img, spots, n_bands, sigma)."""
    r = 1 if sigma >= 0.25 else 0
    step = 2 * r + 2
    rng = np.random.default_rng([seed, rows, cols, 41])
    f = _background(rng, rows, cols)
    ys = np.linspace(20, rows - 21, n_spots)
    spots = np.stack([np.where(np.arange(n_spots) % 2 == 0, 10.0, cols - 11.0), np.floor(ys) + 0.5], 1).reshape(-1, 2)
    _paste_spots(f, spots, seed)
    n = 0
    for y in range(r, rows - r, step):
        if np.all(np.abs(spots[:, 1] - y) > 8):
            f[y, int(rng.integers(2, cols - 2))] = 255
            n += 1
    f.setflags(write=False)
    return dict(img=f, spots=spots, n_bands=n, sigma=sigma)


def count_bands(mask):
    """Maximal runs of non-empty rows of a mask (numpy; for checking band_frame's bound against the oracle's blurred mask)."""
    act = np.asarray(mask).any(axis=1).astype(np.int8)
    return int(((act[1:] == 1) & (act[:-1] == 0)).sum() + int(act[0]))


# ---- ROIs beyond (2048, 1200) on the full-size frame ---------------------------------------------------------------------
FULL_ROIS = [(3900, 4000, 100, 96), (2040, 4080, 16, 16),
             (2000, MAX_ROWS - 1, 2000, 1),       # one row: the last
             (MAX_COLS - 1, 2048, 1, 2048)]       # one column: the last


# ---- the C2 marker set seen in the far quarter of a full-size frame ------------------------------------------------------

def far_quarter_scene(n=2, seed=7, rows=MAX_ROWS, cols=MAX_COLS, margin=40.0):
    """n poses of synth.M5 whose (distorted) LEDs all lie in x >= cols / 2, y >= rows / 2 of a rows x cols frame of
    synth.camera_for(rows, cols), at least `margin` from its edges and 12 px apart, and the frames: background
    integers(0, 30), the spots in patches (sigma 2.0, as the 1920 x 1200 configuration draws them).
    -> dict(frames (n, rows, cols), T_true, px (n, 5, 2), K, D, markers)."""
    K, D = synth.camera_for(rows, cols)
    rng = np.random.default_rng([seed, 53])
    Ts, pxs = [], []
    while len(Ts) < n:
        T = np.eye(4)
        T[:3, :3] = synth.rodrigues(rng.normal(size=3), rng.uniform(0.0, 0.8))
        T[:3, 3] = [rng.uniform(0.1, 0.45), rng.uniform(0.08, 0.3), rng.uniform(0.9, 1.6)]
        px = synth.distort_px(synth.project(T, synth.M5, K), K, D)
        d = np.linalg.norm(px[:, None] - px[None], axis=-1) + np.eye(5) * 1e9
        if (px[:, 0].min() >= cols / 2 + margin and px[:, 0].max() <= cols - 1 - margin and px[:, 1].min() >= rows / 2 + margin
                and px[:, 1].max() <= rows - 1 - margin and d.min() >= 12.0):
            Ts.append(T)
            pxs.append(px)
    frames = np.empty((n, rows, cols), np.uint8)
    for i in range(n):
        frames[i] = _paste_spots(_background(np.random.default_rng([seed, i, 59]), rows, cols), pxs[i], seed + i, 2.0)
    return dict(frames=frames, T_true=np.array(Ts), px=np.array(pxs), K=K, D=D, markers=synth.M5)
