"""CPU witness of the Bayer and YUV 4:2:2 decodes of mpe_convert_to_mono8 (include/mpe.h, MPE_ENC_BAYER_* and
MPE_ENC_YUV422*): a numpy restatement written from the rule as the header states it, in two forms — a literal
row-by-row loop in the statement order of OpenCV's scalar Bayer2Gray, and a vectorised colour-map form — that must agree
(test_sensor_encodings.py asserts it on all sizes 1 x 1 .. 8 x 8 and all four patterns).

UNPINNED: nothing reference-held fixes these bytes.  The reference calls cv_bridge::toCvCopy(msg, MONO8), no OpenCV
was at hand to run it against, and OpenCV's SIMD path of this conversion rounds per term and can differ from its scalar
path by one gray level.  What this file pins is the rule of the header, stated twice, and its hand-checked known
answers (KAT_*)."""
import numpy as np

W_R, W_G, W_B = 4899, 9617, 1868
BAYER = {"bayer_rggb8": "RGGB", "bayer_bggr8": "BGGR", "bayer_gbrg8": "GBRG", "bayer_grbg8": "GRBG"}
YUV_Y_BYTE = {"yuv422": 1, "yuv422_yuy2": 0}
BPP = dict({k: 1 for k in BAYER}, yuv422=2, yuv422_yuy2=2)

KAT_IMAGE = np.array([[7, 108, 209, 54, 155],
                      [44, 198, 96, 250, 148],
                      [81, 32, 239, 190, 141],
                      [118, 122, 126, 130, 134]], np.uint8)
# output rows 1 .. 2, columns 1 .. 3
KAT_INTERIOR = {"bayer_rggb8": [[104, 149, 156], [85, 157, 190]],
                "bayer_bggr8": [[116, 149, 168], [85, 145, 190]],
                "bayer_gbrg8": [[145, 171, 197], [126, 186, 171]],
                "bayer_grbg8": [[145, 171, 197], [114, 186, 183]]}


def bayer_to_gray_loop(img, encoding):
    """The literal form.  As OpenCV's scalar loop walks it: per interior row, the weight of the row's own non-green
    colour and of the other one, and whether the row starts (at column 1) on a green site, alternating from there; then
    the first and last column of the row from their neighbours, and at the end the first and last row from theirs."""
    img = np.asarray(img, np.uint8)
    rows, cols = img.shape
    out = np.zeros((rows, cols), np.uint8)
    if rows < 3 or cols < 3:
        return out
    pat = BAYER[encoding]
    w = {"R": W_R, "G": W_G, "B": W_B}
    s = img.astype(np.int64)
    for y in range(1, rows - 1):
        row_colour = pat[2 * (y & 1)] if pat[2 * (y & 1)] != "G" else pat[2 * (y & 1) + 1]   # R or B: this row's
        other = "B" if row_colour == "R" else "R"                                            # ... the rows' above / below
        green = pat[2 * (y & 1) + 1] == "G"                                                  # is column 1 a green site
        for x in range(1, cols - 1):
            c = s[y, x]
            if green:
                t = (w[other] * (s[y - 1, x] + s[y + 1, x]) + w[row_colour] * (s[y, x - 1] + s[y, x + 1])
                     + 2 * W_G * c + (1 << 14)) >> 15
            else:
                t = (w[other] * (s[y - 1, x - 1] + s[y - 1, x + 1] + s[y + 1, x - 1] + s[y + 1, x + 1])
                     + W_G * (s[y - 1, x] + s[y + 1, x] + s[y, x - 1] + s[y, x + 1])
                     + 4 * w[row_colour] * c + (1 << 15)) >> 16
            out[y, x] = t
            green = not green
        out[y, 0] = out[y, 1]
        out[y, cols - 1] = out[y, cols - 2]
    out[0] = out[1]
    out[rows - 1] = out[rows - 2]
    return out


def bayer_to_gray(img, encoding):
    """The colour-map form, vectorised over leading dimensions: every pixel times the weight of the colour the pattern
    gives it; a green site sums its four edge neighbours and twice itself (>> 15), a red or blue site all eight
    neighbours and four times itself (>> 16); output pixel (r, c) is the value at (clamp(r, 1, rows - 2),
    clamp(c, 1, cols - 2))."""
    img = np.asarray(img, np.uint8)
    rows, cols = img.shape[-2:]
    if rows < 3 or cols < 3:
        return np.zeros(img.shape, np.uint8)
    pat = BAYER[encoding]
    yy, xx = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    colour = np.array(list(pat))[2 * (yy & 1) + (xx & 1)]
    weight = np.where(colour == "R", W_R, np.where(colour == "G", W_G, W_B)).astype(np.int64)
    p = img.astype(np.int64) * weight
    mid = p[..., 1:-1, 1:-1]
    edges = p[..., :-2, 1:-1] + p[..., 2:, 1:-1] + p[..., 1:-1, :-2] + p[..., 1:-1, 2:]
    diags = p[..., :-2, :-2] + p[..., :-2, 2:] + p[..., 2:, :-2] + p[..., 2:, 2:]
    inner = np.where(colour[1:-1, 1:-1] == "G", (edges + 2 * mid + (1 << 14)) >> 15, (diags + edges + 4 * mid + (1 << 15)) >> 16)
    ry = np.clip(np.arange(rows), 1, rows - 2) - 1
    rx = np.clip(np.arange(cols), 1, cols - 2) - 1
    return inner[..., ry[:, None], rx[None, :]].astype(np.uint8)


def yuv422_to_gray(raw, encoding):
    """raw (..., rows, cols, 2) uint8: the pixel's Y byte."""
    return np.ascontiguousarray(np.asarray(raw, np.uint8)[..., YUV_Y_BYTE[encoding]])


def to_mono8(raw, encoding):
    """Frames in `encoding` -> mono8: (..., rows, cols) for Bayer, (..., rows, cols, 2) for YUV 4:2:2."""
    return bayer_to_gray(raw, encoding) if encoding in BAYER else yuv422_to_gray(raw, encoding)


def mosaic(gray, encoding, seed, noise=6):
    """Mono8 frames (..., rows, cols) as sensor frames of `encoding` whose decode stays close to them: every Bayer site
    (every Y byte) is the gray value plus seeded noise in [-noise, noise], clipped; U and V are random.
    -> (..., rows, cols) for Bayer, (..., rows, cols, 2) for YUV."""
    rng = np.random.default_rng([seed, sorted(BPP).index(encoding)])
    gray = np.asarray(gray)
    y = np.clip(gray.astype(np.int64) + rng.integers(-noise, noise + 1, gray.shape), 0, 255).astype(np.uint8)
    if encoding in BAYER:
        return y
    uv = rng.integers(0, 256, gray.shape).astype(np.uint8)
    return np.ascontiguousarray(np.stack([uv, y] if YUV_Y_BYTE[encoding] else [y, uv], -1))
