"""GPU tests of the wide path — frames and detection sets of 65 .. 256 points: mpe_detect_batch_wide and
mpe_estimate_batch_wide (what a caller with frames uses), the stage entries mpe_vote_batch_wide and
mpe_solve_bruteforce_batch_wide, and the C++ facade's setWideFrames — against the CPU oracle, whose find_leds, vote and
initialise + optimisePose take any count.  Four markers in the stage tests (the oracle's vote costs microseconds per
hypothesis on one core), five in the frame tests, whose oracle records are committed goldens."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from rpg_monocular_pose_estimator_amd import synth
import rpg_monocular_pose_estimator_amd as mpe
from util import pose_diff, POS_TOL_M, ROT_TOL_RAD

pytestmark = pytest.mark.gpu

ROWS, COLS = 480, 752
M4 = synth.M5[:4]
TOL = 5.0
POSE_TOL = 0.02
# The issue's batch is 65, 66, 100 and 129 detections, with 120 in place of 129 when the oracle needs more than ten
# seconds for 129: measured on the development machine it needs 27.7 s for 129 / 4 (8.4 M hypotheses, each walking
# 126 detections for up to four roots; 19.3 s for 120, 9.5 s for 100, 2.3 s for 65), so 120 it is.  65 sits just past
# a 64-bit mask word; 129 would have sat past the second one — the wide kernel walks the detections and keeps no
# mask, and the 256-point golden below covers all four words.
SIZES = (65, 66, 100, 120)
NARROW = 41
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide", "wide_256x4.npz")


def _scene(rng, n, K, D):
    """A demo scene (4 LEDs of a random pose) + distractor spots, n spots in all, >= 12 px apart — drawn the way
    test_gpu_parity._wide_frame draws its frames; the spot centres themselves are the detections."""
    for _ in range(50):
        _, spots = synth.sample_scene(rng, M4, K, D, ROWS, COLS, n_distractors=n - len(M4))
        if len(spots) == n:
            return np.ascontiguousarray(spots[rng.permutation(n)])
    raise AssertionError("could not place %d spots" % n)


GRID_ROWS, GRID_COLS = 198, 208          # 18 x 17 cells of 11 x 12 pixels
E2E_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide", "wide_e2e.npz")
E2E_SEED, E2E_WIDE = 70130, {1: 70, 5: 130}


def grid_frame(rng, n):
    """n small spots (4 x 5 pixels, one gray level each) on a jittered grid: every one passes the demo shape filter, and
    the 6 dark pixels between neighbours keep their blurred masks apart."""
    f = np.zeros((GRID_ROWS, GRID_COLS), np.uint8)
    for c in rng.permutation((GRID_ROWS // 11) * (GRID_COLS // 12))[:n]:
        r, q = divmod(int(c), GRID_COLS // 12)
        y, x = 11 * r + 2 + rng.integers(0, 2), 12 * q + 2 + rng.integers(0, 3)
        f[y:y + 4, x:x + 5] = rng.integers(200, 256)
    return f


E2E_ROWS, E2E_COLS, E2E_TOL, E2E_SIGMA = 1200, 1920, 0.3, 3.0


def pose_scene(rng, markers, n, K, D, rows, cols, sep, keep, exact):
    """The LEDs of a random pose + distractor spots, n in all, the distractors `keep` px away from every LED and `sep`
    px from each other — far enough from the body's projections for the true rows to win the vote at a small
    back-projection tolerance.  exact: the LEDs' pinhole projections (detections given as points), else their distorted
    pixel positions (spots to render)."""
    while True:
        T, px = synth.sample_scene(rng, markers, K, D, rows, cols, n_distractors=0, min_sep=sep, margin=sep)
        spots = synth.project(T, markers, K) if exact else px.copy()
        led = spots.copy()
        for _ in range(20000):
            if len(spots) == n:
                return T, spots
            c = np.array([rng.uniform(sep, cols - 1 - sep), rng.uniform(sep, rows - 1 - sep)])
            if np.linalg.norm(led - c, axis=1).min() >= keep and np.linalg.norm(spots - c, axis=1).min() >= sep:
                spots = np.vstack([spots, c])


def e2e_frames():
    """8 frames of 1920 x 1200, two of them wide: 70 and 130 spots of a real 5-marker pose plus distractors.  Large
    frames, large spots (sigma 3: centroids good to 0.1 px) and a back-projection tolerance of 0.3 px: at 752 x 480 and
    the demo's 5 px the accidental votes of 65 distractors bury the body's — the oracle finds no pose in such a frame, and
    a test that only ever compares status 1 cannot see a wrong hand-over.  Here the oracle initialises the 70-spot frame."""
    K, D = synth.camera_for(E2E_ROWS, E2E_COLS)
    rng = np.random.default_rng(E2E_SEED)
    plain = synth.make_frames("C4", 8, seed=E2E_SEED)["frames"]
    frames = []
    for i in range(8):
        if i not in E2E_WIDE:
            frames.append(plain[i])
            continue
        _, spots = pose_scene(rng, synth.M5, E2E_WIDE[i], K, D, E2E_ROWS, E2E_COLS, 30.0, 60.0, False)
        frames.append(synth.render_frame(rng, spots, E2E_ROWS, E2E_COLS, spot_sigma=E2E_SIGMA))
    return np.ascontiguousarray(np.stack(frames)), K, D


@pytest.fixture(scope="module")
def sets(orc):
    """The detection sets of the module and the oracle's answer for each (computed once, side by side on threads: the
    oracle's C entry releases the interpreter lock).  This set-up is the module's cost: about 10 s of wall time on 16
    cores — the 120-detection pass alone is 19 s of one slower core — against well under 2 s for every test body."""
    K, D = synth.camera_for(ROWS, COLS)
    rng = np.random.default_rng(65)
    dets = {n: _scene(rng, n, K, D) for n in SIZES + (NARROW,)}
    # spots nowhere near any projection: a lattice 1e5 px wide, a million pixels off the image — no back-projection
    # lands within 5 px of one
    lat = 1e6 + np.stack(np.meshgrid(np.arange(11.0), np.arange(6.0)), -1).reshape(-1, 2) * 1e5 + rng.uniform(-1e3, 1e3, (66, 2))
    dets["zero"] = np.ascontiguousarray(lat)
    dets["three"] = np.ascontiguousarray(dets[65][:3])
    dets["clean"] = _scene(rng, 5, K, D)   # (4 LEDs and one distractor: a set that initialises, for the pose branch)
    # a WIDE set that initialises: the exact projections of a pose among 66 distractors kept 40 px away from them, voted
    # at POSE_TOL = 0.02 px — at the demo's 5 px the accidental votes of so many distractors bury the body's four per row
    prng = np.random.default_rng(7004)
    _, pts = pose_scene(prng, M4, 70, K, D, ROWS, COLS, 12.0, 40.0, True)
    dets["pose70"] = np.ascontiguousarray(pts[prng.permutation(70)])
    tol = {k: (POSE_TOL if k == "pose70" else TOL) for k in dets}
    keys = list(dets)
    with ThreadPoolExecutor(len(keys)) as ex:
        refs = list(ex.map(lambda k: orc.solve_bruteforce(dets[k], M4, K, orc.make_params(back_projection_pixel_tolerance=tol[k])),
                           keys))
    return dict(K=K, dets=dets, ref=dict(zip(keys, refs)))


@pytest.fixture()
def arith(hip):
    yield lambda a: hip.set_option("vote_arith", a)
    hip.set_option("vote_arith", 3)
    hip.set_option("wide_block_cap", 0)


def test_vote_histograms_equal_the_oracle(hip, sets, arith):
    """mpe_vote_batch_wide over one batch of 65, 66, 100 and 120 detections and one narrow set: integer-equal to the
    oracle's vote under vote_arith 3, 1, 4 and 0 (3 = 4 and 1 = 0 follow); the narrow set's rows are mpe_vote_batch's."""
    keys = list(SIZES) + [NARROW]
    batch = [sets["dets"][k] for k in keys]
    got = {}
    for a in (3, 1, 4, 0):
        arith(a)
        got[a] = hip.vote_batch_wide(batch, M4, sets["K"], TOL)
        if a in (3, 1):
            narrow = hip.vote_batch([sets["dets"][NARROW]], M4, sets["K"], TOL)[0]
            assert np.array_equal(got[a][-1], narrow), a
    for a in (3, 1, 4, 0):
        for k, h in zip(keys, got[a]):
            ref = sets["ref"][k]["hist"]
            assert h.shape == ref.shape == (k, 4)
            assert np.array_equal(h, ref), (a, k, np.argwhere(h != ref)[:6])
    for x, y in ((3, 4), (1, 0)):
        assert all(np.array_equal(p, q) for p, q in zip(got[x], got[y]))


def test_histogram_does_not_depend_on_the_partition(hip, sets, arith):
    """The 100-detection set voted by ONE block (option "wide_block_cap" = 1) and by the default share of the chip."""
    d = [sets["dets"][100]]
    hip.set_option("wide_block_cap", 1)
    assert hip.get_option("wide_block_cap") == 1
    one = hip.vote_batch_wide(d, M4, sets["K"], TOL)[0]
    hip.set_option("wide_block_cap", 0)
    many = hip.vote_batch_wide(d, M4, sets["K"], TOL)[0]
    assert np.array_equal(one, many) and np.array_equal(one, sets["ref"][100]["hist"])


def _check_solved(rec, hist, corr, ref, n_det, what):
    n_c = int(ref["n_corr"])
    assert np.array_equal(hist[:n_det, :4], ref["hist"]), what
    assert not hist[n_det:].any() and not hist[:, 4:].any(), what
    assert rec["status"] == ref["status"] and rec["n_det"] == n_det and rec["n_corr"] == n_c, (what, rec["status"], rec["n_corr"])
    assert np.array_equal(corr[:n_c], np.asarray(ref["corr"]).reshape(-1, 2)[:n_c]) and not corr[n_c:].any(), (what, corr[:n_c])
    if ref["status"] == 0:
        dp, dr = pose_diff(rec["T"], ref["T"])
        print(what, "pose diff", dp, dr)
        assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (what, dp, dr)
        assert np.allclose(rec["cov"].reshape(6, 6), ref["cov"], rtol=1e-6, atol=1e-12), what
    else:
        assert np.array_equal(rec["T"].reshape(4, 4), np.eye(4)) and not rec["cov"].any(), what


def test_solve_equals_the_oracle(hip, sets):
    """mpe_solve_bruteforce_batch_wide over the same sets + one with an all-zero histogram and one of 3 detections:
    status, counts and rows (in the caller's indices) equal initialise + optimisePose of the oracle, pose within the
    project's tolerance, covariance at test_gpu_parity's rtol.  (The set whose rows name one detection through two
    markers is the 256-point golden below: its oracle pass is the one that could be searched for such rows.)"""
    keys = list(SIZES) + [NARROW, "clean", "zero", "three"]
    before = hip.get_option("wide_frames")
    rec, hist, corr = hip.solve_bruteforce_batch_wide([sets["dets"][k] for k in keys], M4, sets["K"],
                                                      mpe.demo_params(back_projection_pixel_tolerance=TOL))
    assert hip.get_option("wide_frames") == before + 5   # (the sets of more than 64 points: 65, 66, 100, 120, "zero")
    for i, k in enumerate(keys):
        _check_solved(rec[i], hist[i], corr[i], sets["ref"][k], len(sets["dets"][k]), k)
    assert not sets["ref"]["zero"]["hist"].any() and sets["ref"]["zero"]["status"] == 1 and rec[-2]["n_corr"] == 0
    assert sets["ref"]["three"]["status"] == 1 and rec[-1]["n_corr"] == 0
    assert sets["ref"]["clean"]["status"] == 0   # (the pose branch of the comparison was taken)
    # ... and for a set of more than 64 points: pose, covariance and rows whose detection indices lie all over the set
    ref = sets["ref"]["pose70"]
    assert ref["status"] == 0 and ref["n_corr"] == 4 and np.asarray(ref["corr"])[:, 1].max() > 16
    rec, hist, corr = hip.solve_bruteforce_batch_wide([sets["dets"]["pose70"]], M4, sets["K"],
                                                      mpe.demo_params(back_projection_pixel_tolerance=POSE_TOL))
    _check_solved(rec[0], hist[0], corr[0], ref, 70, "pose70")
    assert np.array_equal(hip.vote_batch_wide([sets["dets"]["pose70"]], M4, sets["K"], POSE_TOL)[0], ref["hist"])


def test_256_detections_against_the_golden(hip, arith):
    """One 256-detection / 4-marker set whose histogram and record the oracle computed once
    (tests/golden/wide/make_wide_golden.py: minutes of CPU).  Its winning rows name detection 256 — a 1-based index no
    byte holds — and name one detection through two markers (only the winning column is zeroed)."""
    g = np.load(GOLDEN)
    n_c = int(g["n_corr"])
    rows = g["corr"][:n_c]
    assert len(g["det"]) == 256 and (rows[:, 1] >= 255).any() and len(set(rows[:, 1].tolist())) < n_c   # (the fixture's point)
    ref = dict(hist=g["hist"], status=int(g["status"]), n_corr=n_c, corr=g["corr"], T=g["T"], cov=g["cov"])
    P = mpe.demo_params(back_projection_pixel_tolerance=float(g["tol"]))
    for a in (3, 1):
        arith(a)
        h = hip.vote_batch_wide([g["det"]], g["markers"], g["K"], float(g["tol"]))[0]
        assert np.array_equal(h, g["hist"]), (a, np.argwhere(h != g["hist"])[:6])
        rec, hist, corr = hip.solve_bruteforce_batch_wide([g["det"]], g["markers"], g["K"], P)
        _check_solved(rec[0], hist[0], corr[0], ref, 256, "golden/%d" % a)


def test_detection_equals_the_oracle(hip, orc):
    """mpe_detect_batch_wide on frames of 70, 130 and 256 small spots: the oracle's find_leds count and centres bit for
    bit, in its order, status 0; 300 spots: MPE_FRAME_TOO_MANY_DETECTIONS (-10, as include/mpe.h documents for anything
    above 256 passing blobs) with n = 256 and the first 256 of the oracle's order; mpe_detect_batch on the same frames
    still answers -10 with its first 64.  Both kernels of the general tier."""
    K, D = synth.camera_for(GRID_ROWS, GRID_COLS)
    rng = np.random.default_rng(70)
    counts = (70, 130, 256, 300)
    frames = np.stack([grid_frame(rng, n) for n in counts])
    Po, Ph = orc.make_params(), mpe.demo_params()
    ref = [orc.find_leds(f, Po, K, D) for f in frames]
    assert [len(u) for u, _ in ref] == list(counts)
    try:
        for lds in (0, 1):
            hip.set_option("general_lds", lds)
            got = hip.detect_batch_wide(frames, K, D, Ph)
            for i, (und, dist) in enumerate(ref):
                k = min(len(und), mpe.WIDE_DETECTIONS)
                assert got["status"][i] == (0 if len(und) <= mpe.WIDE_DETECTIONS else -10), (lds, i, got["status"][i])
                assert got["n"][i] == k, (lds, i, got["n"][i])
                assert np.array_equal(got["dist_xy"][i][:2 * k].reshape(-1, 2), dist[:k]), (lds, i)
                assert np.array_equal(got["undist_xy"][i][:2 * k].reshape(-1, 2), und[:k]), (lds, i)
            narrow = hip.detect_batch(frames, K, D, Ph)
            for i, (und, dist) in enumerate(ref):
                assert narrow["status"][i] == -10 and narrow["n"][i] == mpe.MAX_DETECTIONS, (lds, i)
                assert np.array_equal(narrow["dist_xy"][i][:2 * 64].reshape(-1, 2), dist[:64]), (lds, i)
    finally:
        hip.set_option("general_lds", 0)


@pytest.mark.parametrize("on_device", [False, True], ids=["host_frames", "device_frames"])
def test_estimate_batch_wide_end_to_end(hip, on_device):
    """mpe_estimate_batch_wide over 8 frames, two of them wide (70 and 130 spots of a real 5-marker pose + distractors):
    the six ordinary records are byte-identical to mpe_estimate_batch's, the two wide ones match the oracle's
    estimateBodyPose (tests/golden/wide/make_wide_e2e_golden.py: its vote of the 130-spot frame takes more than a minute),
    "wide_frames" advances by 2."""
    import hashlib
    g = np.load(E2E_GOLDEN)
    frames, K, D = e2e_frames()
    assert [hashlib.sha1(f.tobytes()).hexdigest() for f in frames] == [str(x) for x in g["sha1"]], "frame generator drifted"
    assert [int(g["n_det"][i]) for i in sorted(E2E_WIDE)] == [E2E_WIDE[i] for i in sorted(E2E_WIDE)]
    assert any(g["status"][i] == 0 for i in E2E_WIDE)   # (the oracle initialises a wide frame: its pose is compared)
    P = mpe.demo_params(back_projection_pixel_tolerance=float(g["tol"]))
    arg = frames
    if on_device:
        import torch
        arg = torch.from_numpy(frames).cuda()
    plain = hip.estimate_batch(arg, synth.M5, K, D, P)
    before = hip.get_option("wide_frames")
    wide = hip.estimate_batch_wide(arg, synth.M5, K, D, P)
    assert hip.get_option("wide_frames") == before + 2
    for i in range(8):
        if i in E2E_WIDE:
            assert plain["status"][i] == -10
            assert wide["status"][i] == g["status"][i] and wide["n_det"][i] == g["n_det"][i] and wide["n_corr"][i] == g["n_corr"][i], \
                (i, wide["status"][i], wide["n_det"][i], wide["n_corr"][i])
            if g["status"][i] == 0:
                dp, dr = pose_diff(wide["T"][i], g["T"][i])
                print("frame", i, "pose diff", dp, dr)
                assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (i, dp, dr)
        else:
            assert plain["status"][i] == g["status"][i]
            assert wide[i].tobytes() == plain[i].tobytes(), i


def test_facade_switch_takes_the_wide_entries(hip, sets, tmp_path):
    """compat PoseEstimator::setWideFrames.  Off (the default): initialise() on 70 image points and estimateBodyPose on a
    70-blob frame raise the capacity exception, as today.  On: initialise() + optimiseAndUpdatePose give the oracle's rows,
    pose and covariance for the point set, and estimateBodyPose the oracle's pose for the frame."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "compat")])
    g = np.load(E2E_GOLDEN)
    frames, Kf, Df = e2e_frames()
    wide_i = [i for i in sorted(E2E_WIDE) if g["status"][i] == 0][0]
    yaml4, yaml5, pts, raw = (str(tmp_path / n) for n in ("m4.yaml", "m5.yaml", "points.txt", "frame.raw"))
    for path, markers in ((yaml4, M4), (yaml5, synth.M5)):
        with open(path, "w") as fh:
            fh.write("marker_positions:\n")
            for m in markers:
                fh.write("  - x: %.17g\n    y: %.17g\n    z: %.17g\n" % tuple(m))
    np.savetxt(pts, sets["dets"]["pose70"], fmt="%.17g")
    frames[wide_i].tofile(raw)
    exe = os.path.join(root, "compat", "facade_selftest")

    def run(args):
        out = subprocess.run([exe, "wide"] + args, capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stdout[-800:], out.stderr[-800:])
        return out.stdout.splitlines()

    def state(lines, what):
        vals = {ln.split()[1]: np.array(ln.split()[2:], float) for ln in lines if ln.startswith(what + " ") and
                ln.split()[1] in ("rows", "pose", "cov")}
        return vals["rows"].astype(int).reshape(-1, 2), vals["pose"].reshape(4, 4), vals["cov"].reshape(6, 6)

    cam = lambda K: "%.17g %.17g %.17g %.17g" % (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    # the point set: camera without distortion (the points are pinhole projections)
    lines = run(["--markers", yaml4, "--camera", cam(sets["K"]), "--points", pts, "--tol", repr(POSE_TOL)])
    assert any(ln.startswith("points wide=0 exception") for ln in lines), lines
    assert "points wide=1 initialise 1" in lines, lines
    ref = sets["ref"]["pose70"]
    rows, T, cov = state(lines, "points")
    assert np.array_equal(rows, np.asarray(ref["corr"]).reshape(-1, 2))
    dp, dr = pose_diff(T, ref["T"])
    assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (dp, dr)
    assert np.allclose(cov, ref["cov"], rtol=1e-6, atol=1e-12)
    # the frame
    lines = run(["--markers", yaml5, "--camera", cam(Kf), "--dist", " ".join("%.17g" % v for v in Df), "--frame", raw,
                 "--rows", str(E2E_ROWS), "--cols", str(E2E_COLS), "--frame-tol", repr(float(g["tol"]))])
    assert any(ln.startswith("frame wide=0 exception") for ln in lines), lines
    n = int(g["n_det"][wide_i])
    assert "frame wide=1 estimateBodyPose 1 points %d centres %d" % (n, n) in lines, lines
    rows, T, cov = state(lines, "frame")
    assert len(rows) == g["n_corr"][wide_i]
    dp, dr = pose_diff(T, g["T"][wide_i])
    assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (dp, dr)
    assert np.allclose(cov, g["cov"][wide_i].reshape(6, 6), rtol=1e-6, atol=1e-12)


def test_usage_errors_leave_the_handle_usable(hip, sets):
    lib = hip._lib
    dp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_uint32)
    W = mpe.WIDE_DETECTIONS
    xy = np.zeros((2, W, 2))
    xy[0, :5] = sets["dets"][65][:5]
    nd = np.array([5, 0], np.int32)
    K = np.ascontiguousarray(sets["K"], float).reshape(9)
    m = np.ascontiguousarray(M4, float)
    P = mpe.demo_params()
    out = np.zeros(2, mpe.RESULT_DTYPE)
    hist = np.zeros((2, W, mpe.MAX_MARKERS), np.uint32)
    good = dict(h=hip._h, xy=xy.ctypes.data_as(dp), nd=nd.ctypes.data_as(ip), n=2, m=m.ctypes.data_as(dp), nm=4,
                K=K.ctypes.data_as(dp), p=C.byref(P), out=C.c_void_p(out.ctypes.data), hist=hist.ctypes.data_as(up))

    def solve(**kw):
        a = dict(good, **kw)
        return lib.mpe_solve_bruteforce_batch_wide(a["h"], a["xy"], a["nd"], a["n"], a["m"], a["nm"], a["K"], a["p"], a["out"],
                                                   a["hist"], None)

    def vote(**kw):
        a = dict(good, **kw)
        return lib.mpe_vote_batch_wide(a["h"], a["xy"], a["nd"], a["n"], a["m"], a["nm"], a["K"], 5.0, a["hist"])

    bad_counts = [np.array([5, -1], np.int32), np.array([W + 1, 5], np.int32)]
    for call in (solve, vote):
        for null in ("h", "xy", "nd", "m", "K"):
            assert call(**{null: None}) == -1, (call.__name__, null)
        assert call(n=-1) == -1
        for bad in bad_counts:
            assert call(nd=bad.ctypes.data_as(ip)) == -1
        assert call(nm=0) == -1 and call(nm=17) == -1
        assert call(n=0) == 0
    assert solve(p=None) == -1 and solve(out=None) == -1 and vote(hist=None) == -1
    hip.set_option("vote_arith", 2)
    try:
        assert solve() == -3 and vote() == -3            # MPE_ERR_UNSUPPORTED: the fast arithmetic has no strict form
    finally:
        hip.set_option("vote_arith", 3)
    # an un-collected lock-step submission on the handle
    img = np.zeros((64, 64), np.uint8)
    item = mpe.binding.TrackItem(img.ctypes.data, 0, 0, 64, 64, None)
    Dz = np.zeros(5)
    rc = lib.mpe_track_step_batch_submit(hip._h, C.byref(item), 1, 64, 64, C.c_size_t(64), C.byref(P), K.ctypes.data_as(dp),
                                         Dz.ctypes.data_as(dp), 5, m.ctypes.data_as(dp), 4)
    assert rc == 0
    try:
        assert solve() == -1 and vote() == -1
    finally:
        assert lib.mpe_track_step_batch_cancel(hip._h) == 0
    # an un-collected streaming submission on the handle
    import torch
    d_frames = torch.zeros((1, 64, 64), dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(mpe.RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    hip.estimate_batch_device_submit(d_frames.data_ptr(), 1, 64, 64, M4, sets["K"], Dz, P, d_res.data_ptr())
    fr = np.zeros((1, 64, 64), np.uint8)
    dw = np.zeros(1, mpe.DETECTIONS_WIDE_DTYPE)
    res1 = np.zeros(1, mpe.RESULT_DTYPE)

    def detect(frames=fr.ctypes.data, dets=dw.ctypes.data, n=1, k=K.ctypes.data_as(dp), p=C.byref(P)):
        return lib.mpe_detect_batch_wide(hip._h, C.c_void_p(frames), n, 64, 64, C.c_size_t(64), C.c_size_t(4096), 0, k,
                                         Dz.ctypes.data_as(dp), 5, p, C.c_void_p(dets))

    def estimate(frames=fr.ctypes.data, res=res1.ctypes.data, n=1, nm=4, p=C.byref(P)):
        return lib.mpe_estimate_batch_wide(hip._h, C.c_void_p(frames), n, 64, 64, C.c_size_t(64), C.c_size_t(4096), 0,
                                           m.ctypes.data_as(dp), nm, K.ctypes.data_as(dp), Dz.ctypes.data_as(dp), 5, p,
                                           C.c_void_p(res))
    try:
        assert solve() == -1 and vote() == -1 and detect() == -1 and estimate() == -1
    finally:
        hip.estimate_batch_device_collect()
        hip.synchronize()
    # the frame-taking entries: null pointers, counts, markers
    assert detect(frames=None) == -1 and detect(dets=None) == -1 and detect(n=-1) == -1 and detect(k=None) == -1
    assert detect(p=None) == -1 and detect(n=0) == 0
    assert estimate(frames=None) == -1 and estimate(res=None) == -1 and estimate(n=-1) == -1 and estimate(p=None) == -1
    assert estimate(nm=0) == -1 and estimate(nm=17) == -1 and estimate(n=0) == 0
    assert detect() == 0 and dw["n"][0] == 0 and dw["status"][0] == 0
    assert estimate() == 0 and res1["status"][0] == 1
    # ... and the handle works
    assert solve() == 0 and out["status"].tolist() == [1, 1] and out["n_det"].tolist() == [5, 0]
    assert vote() == 0
