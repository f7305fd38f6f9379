"""A numpy witness of the rig's partial-view tracking step (include/mpe.h, mpe_rig_track_batch), written in ANOTHER
formulation than the device code: per camera a dense distance matrix (markers x detections) with np.argmin for the
nearest detection, the one-marker-per-detection rule by sorting the candidates by (detection, distance, marker) and
keeping the head of every group, witness_rig.rig_optimise_pose (the other chain rule, np.linalg.solve) for the
refinement, and the projection as K (E T p) with the division last.

Comparisons at a tolerance are knife edges: where a candidate distance or a final residual lies within `margin` of the
tolerance it is compared with, or two competing distances lie within `margin` of each other without being equal, two
correct implementations may disagree.  The witness measures these margins ON ITS OWN NUMBERS and raises KnifeEdge; the
generators below re-draw such a problem and count how often they had to."""
import numpy as np

import witness_rig

MARGIN = 1e-6


class KnifeEdge(Exception):
    pass


def _near(a, b, margin):
    """a and b differ by less than margin without being equal (an exact tie is decided by rule, not by rounding)"""
    return a != b and abs(a - b) < margin


def project(cameras, T, markers):
    """-> (uv (n_cam, n_mk, 2), visible (n_cam, n_mk))"""
    n_cam, n_mk = len(cameras), len(markers)
    uv = np.full((n_cam, n_mk, 2), np.nan)
    vis = np.zeros((n_cam, n_mk), bool)
    P = np.hstack([np.asarray(markers, float), np.ones((n_mk, 1))])
    for c, (K, E) in enumerate(cameras):
        q = (np.asarray(E, float).reshape(4, 4) @ np.asarray(T, float).reshape(4, 4) @ P.T)[:3]
        h = np.asarray(K, float).reshape(3, 3) @ q
        with np.errstate(all="ignore"):
            uv[c] = (h[:2] / h[2]).T
        vis[c] = (q[2] > 0) & np.isfinite(uv[c]).all(axis=1)
    return uv, vis


def match_round(cameras, T, markers, dets, tol, margin=MARGIN):
    """One round's row set: -> match (n_cam, n_mk) int, 1-based detection or 0."""
    n_cam, n_mk = len(cameras), len(markers)
    uv, vis = project(cameras, T, markers)
    match = np.zeros((n_cam, n_mk), np.int64)
    for c in range(n_cam):
        det = np.asarray(dets[c], float).reshape(-1, 2)
        if len(det) == 0 or not vis[c].any():
            continue
        D = np.sqrt(((uv[c][:, None, :] - det[None, :, :]) ** 2).sum(axis=2))  # (n_mk, n_det)
        cand = []
        for m in range(n_mk):
            if not vis[c, m]:
                continue
            j = int(np.argmin(D[m]))  # (the first minimum)
            d = D[m, j]
            if any(_near(d, o, margin) for o in np.delete(D[m], j)):
                raise KnifeEdge("camera %d marker %d: two detections as near" % (c, m))
            if np.isfinite(tol[c]) and abs(d - tol[c]) < margin:
                raise KnifeEdge("camera %d marker %d: distance at the tolerance" % (c, m))
            if d <= tol[c]:
                cand.append((j, d, m))
        cand.sort()  # by detection, then distance, then marker: the head of a detection's group keeps it
        for k, (j, d, m) in enumerate(cand):
            if k > 0 and cand[k - 1][0] == j:
                continue
            if k + 1 < len(cand) and cand[k + 1][0] == j and _near(cand[k + 1][1], d, margin):
                raise KnifeEdge("camera %d detection %d: two markers as near" % (c, j))
            match[c, m] = j + 1
    return match


def rows_of(match, markers, dets):
    return [(c, np.asarray(markers[m], float), np.asarray(dets[c], float).reshape(-1, 2)[match[c, m] - 1])
            for c in range(match.shape[0]) for m in range(match.shape[1]) if match[c, m]]


def rig_track(cameras, markers, dets, T_pred, tol_match, tol_accept, max_rounds=2, min_rows=4, min_markers=3,
              margin=MARGIN):
    """-> dict(status, T, cov, iterations, match, rounds, rows, distinct_markers, reason, max_residual, rms)"""
    T_pred = np.array(T_pred, float).reshape(4, 4)
    T, cov, iters = T_pred.copy(), np.zeros((6, 6)), 0
    reason, rounds, prev = 0, 0, None
    r = 0
    while True:
        match = match_round(cameras, T, markers, dets, tol_match if r == 0 else tol_accept, margin)
        rows = rows_of(match, markers, dets)
        distinct = int(match.any(axis=0).sum())
        if len(rows) < min_rows:
            reason = 1
            break
        if distinct < min_markers:
            reason = 2
            break
        if r > 0 and np.array_equal(match, prev):
            break
        prev = match
        T, cov, iters, st = witness_rig.rig_optimise_pose(cameras, rows, T)
        rounds = r + 1
        if st != 0:
            reason = 3
            break
        if rounds >= max_rounds:
            break
        r += 1
    worst, rms = 0.0, 0.0
    if reason == 0:
        uv, _ = project(cameras, T, markers)
        res = np.array([np.linalg.norm(np.asarray(dets[c], float).reshape(-1, 2)[match[c, m] - 1] - uv[c, m])
                        for c in range(match.shape[0]) for m in range(match.shape[1]) if match[c, m]])
        tl = np.array([tol_accept[c] for c in range(match.shape[0]) for m in range(match.shape[1]) if match[c, m]])
        if (np.isfinite(tl) & (np.abs(res - tl) < margin)).any():
            raise KnifeEdge("a final residual at the accept tolerance")
        worst, rms = float(res.max()), float(np.sqrt((res ** 2).mean()))
        if not (res <= tl).all():
            reason = 4
    if reason != 0:
        T, cov = T_pred.copy(), np.zeros((6, 6))
    return dict(status=0 if reason == 0 else 1, T=T, cov=cov, iterations=iters, match=match, rounds=rounds,
                rows=int((match != 0).sum()), distinct_markers=distinct, reason=reason, max_residual=worst, rms=rms)


def check_against_witness(rec, match, info, problem, options=None, what=None):
    """rec [RESULT_DTYPE], match (n_cam, n_mk), info [RIG_TRACK_INFO_DTYPE] of one problem against the witness, with the
    criteria of witness_rig.check_against_witness for the refinement (pose 1e-9, covariance rtol 1e-5 / atol 1e-12,
    iterations +-1) and EQUAL match, rounds, reason, row and marker counts.  -> the witness's dict."""
    w = rig_track(*problem, **(options or {}))
    assert np.array_equal(np.asarray(match).reshape(w["match"].shape), w["match"]), (what, match, w["match"])
    assert int(info["reason"]) == w["reason"] and int(info["rounds"]) == w["rounds"], (what, info, w["reason"], w["rounds"])
    assert int(info["rows"]) == w["rows"] and int(info["distinct_markers"]) == w["distinct_markers"], (what, info)
    assert int(rec["status"]) == w["status"] and int(rec["n_corr"]) == w["rows"], what
    assert int(rec["n_det"]) == int((w["match"] != 0).any(axis=1).sum()), what
    assert abs(int(rec["gn_iterations"]) - w["iterations"]) <= 1, (what, int(rec["gn_iterations"]), w["iterations"])
    assert np.abs(rec["T"].reshape(4, 4) - w["T"]).max() <= 1e-9, (what, np.abs(rec["T"].reshape(4, 4) - w["T"]).max())
    assert np.allclose(rec["cov"].reshape(6, 6), w["cov"], rtol=1e-5, atol=1e-12), what
    if w["reason"] in (0, 4):
        assert abs(float(info["max_residual"]) - w["max_residual"]) <= 1e-6 and abs(float(info["rms"]) - w["rms"]) <= 1e-6, what
    else:
        assert float(info["max_residual"]) == 0.0 and float(info["rms"]) == 0.0, what
    if w["status"] != 0:
        assert np.array_equal(rec["T"].reshape(4, 4), np.asarray(problem[3], float).reshape(4, 4)) and not rec["cov"].any(), what
    return w


# ---- problems for the tests (CPU tier and GPU tier draw from the same generators) -----------------------------------
# a problem is the tuple (cameras, markers, dets, T_pred, tol_match, tol_accept) rig_track takes

def random_problem(rng, n_cam=None, n_mk=5, seen=None, clutter=2, noise=0.1, start=(0.004, 0.004), tol=(12.0, 3.0),
                   displace=None, spread=0.25, backwards=None, rig=None):
    """A rig of n_cam cameras (1 - 6 when None) in front of a body of n_mk markers in a cube of half-size `spread`; camera
    c sees seen[c] of them (a count: a random subset; a list: those; None: 2 - n_mk), pixels with `noise` px noise
    rounded through float32 plus clutter (a count or one per camera) stray detections, the list shuffled; T_pred `start`
    (rad, m) off the true pose.  displace = (camera, px): the detection of that camera's first seen LED lies px pixels
    off.  backwards = camera: its extrinsic is turned by pi about y, so every marker is BEHIND it, and its detections
    are where the markers project all the same.  rig = (cameras, markers): these instead of drawn ones.
    -> (problem, T_true)"""
    if rig is not None:
        cameras, markers = list(rig[0]), np.asarray(rig[1], float)
        n_cam, n_mk = len(cameras), len(markers)
    else:
        n_cam = int(rng.integers(1, 7)) if n_cam is None else n_cam
        markers = rng.uniform(-spread, spread, (n_mk, 3))
        cameras = witness_rig.random_cameras(rng, n_cam)
    if backwards is not None:
        K, E = cameras[backwards]
        cameras[backwards] = (K, np.diag([-1.0, 1.0, -1.0, 1.0]) @ E)
    T_true = witness_rig._rigid(rng, rng.uniform(0, 0.6), [rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(1.2, 2.2)])
    if seen is None:
        seen = [int(rng.integers(2, n_mk + 1)) for _ in range(n_cam)]
        if n_cam == 1:
            seen = [max(seen[0], 4)]
    uv = np.zeros((n_cam, n_mk, 2))
    for c, (K, E) in enumerate(cameras):  # (through the plane z = 1 whatever the sign of z)
        q = (E @ T_true @ np.hstack([markers, np.ones((n_mk, 1))]).T)[:3]
        uv[c] = np.stack([K[0, 0] * q[0] / q[2] + K[0, 2], K[1, 1] * q[1] / q[2] + K[1, 2]], axis=1)
    dets = []
    for c in range(n_cam):
        ms = sorted(rng.permutation(n_mk)[:seen[c]]) if np.isscalar(seen[c]) else list(seen[c])
        pts = [uv[c, m] + rng.normal(0, noise, 2) for m in ms]
        if displace is not None and displace[0] == c and ms:
            ang = rng.uniform(0, 2 * np.pi)
            pts[0] = uv[c, ms[0]] + displace[1] * np.array([np.cos(ang), np.sin(ang)])
        n_clutter = clutter if np.isscalar(clutter) else clutter[c]
        pts += [np.array([rng.uniform(0, 752), rng.uniform(0, 480)]) for _ in range(n_clutter)]
        pts = np.array(pts, float).reshape(-1, 2)
        dets.append(pts[rng.permutation(len(pts))].astype(np.float32).astype(np.float64))
    T_pred = witness_rig._rigid(rng, start[0], rng.normal(size=3) * start[1] / np.sqrt(3)) @ T_true
    return (cameras, markers, dets, T_pred, np.full(n_cam, tol[0]), np.full(n_cam, tol[1])), T_true


def draw(rng, options=None, **kw):
    """random_problem, re-drawn while the witness meets a knife edge.  -> (problem, T_true, witness dict, re-draws)"""
    redraws = 0
    while True:
        problem, T_true = random_problem(rng, **kw)
        try:
            return problem, T_true, rig_track(*problem, **(options or {})), redraws
        except KnifeEdge:
            redraws += 1
            assert redraws < 20, "the generator keeps meeting knife edges"


def exact_camera():
    """fx = fy = 400, c = (376, 240), the identity extrinsic: with T_pred = I and markers at z = 1 with binary fractions
    the predicted pixels are exact in any evaluation order."""
    return (np.array([[400.0, 0, 376.0], [0, 400.0, 240.0], [0, 0, 1]]), np.eye(4))


def exact_problem(kind):
    """One exact camera, T_pred = I, the markers m0 .. m3 at the corners (+-0.25, +-0.125, 1) -> pixels (276 | 476, 190 |
    290), m4 = (0, 0, 1) -> (376, 240), m5 = (1/64, 0, 1) -> (382.25, 240); the corners' detections sit 0.5 px beside
    their pixels.  kind:
      "claimed_distinct"   a detection at (378, 240): 2 px from m4, 4.25 px from m5 -> m4 keeps it
      "claimed_higher"     a detection at (381, 240): 5 px from m4, 1.25 px from m5 -> m5 keeps it
      "claimed_tie"        a detection at (379.125, 240): 3.125 px from both -> the lower marker m4 keeps it
      "detection_tie"      m5 left out; detections at (373, 240) and (379, 240), both 3 px from m4 -> the first keeps it
      "detection_tie_swapped"  the same two the other way round
    -> (problem, expected match row of the camera)"""
    mk = [[-0.25, -0.125, 1], [0.25, -0.125, 1], [0.25, 0.125, 1], [-0.25, 0.125, 1], [0, 0, 1], [0.015625, 0, 1]]
    corners = [[276.5, 190.0], [476.0, 190.5], [475.5, 290.0], [276.0, 289.5]]
    if kind.startswith("claimed"):
        x = dict(claimed_distinct=378.0, claimed_higher=381.0, claimed_tie=379.125)[kind]
        det = corners + [[x, 240.0]]
        want = [1, 2, 3, 4, 0, 5] if kind == "claimed_higher" else [1, 2, 3, 4, 5, 0]
    else:
        mk = mk[:5]
        pair = [[373.0, 240.0], [379.0, 240.0]]
        det = (pair[::-1] if kind.endswith("swapped") else pair) + corners
        want = [3, 4, 5, 6, 1]
    problem = ([exact_camera()], np.array(mk, float), [np.array(det, float)], np.eye(4), np.array([12.0]), np.array([6.0]))
    return problem, np.array([want])


def shapes(seed=20241020):
    """The smallest problems at which the step can go wrong.  -> (list of dict(name, problem, options, expect — what the
    WITNESS must say about it: reason, and where given rows / rounds / match), re-draws)"""
    rng = np.random.default_rng(seed)
    out, redraws = [], 0

    def add(name, options, expect, **kw):
        nonlocal redraws
        problem, _, w, n = draw(rng, options, **kw)
        redraws += n
        out.append(dict(name=name, problem=problem, options=options, expect=expect))

    add("1x4", dict(), dict(reason=0, rows=4), n_cam=1, n_mk=4, seen=[4])
    # 256 pairs, four per lane; 16 + 0 + 5 + 8 + 9 * 4 = 65 rows; camera 1 without a detection, camera 2 with 64
    add("16x16", dict(), dict(reason=0, rows=65), n_cam=16, n_mk=16, seen=[16, 0, 5, 8] + [4] * 9 + [0] * 3,
        clutter=[2, 0, 59] + [2] * 13, start=(0.002, 0.001), spread=0.5)
    add("behind", dict(), dict(reason=0, behind=2), n_cam=3, seen=[4, 3, 5], backwards=2, clutter=1)
    add("three_rows", dict(), dict(reason=1, rows=3), n_cam=2, seen=[2, 1], clutter=0)
    add("two_markers", dict(), dict(reason=2, rows=4), n_cam=2, seen=[[1, 3], [1, 3]], clutter=0)
    # a detection 8 px off its LED, inside the match tolerance of 12 px and outside the accept tolerance of 3 px: one round
    # refines over it and fails the accept test; the second round drops it (the row set changes) and refines without it
    for rounds, expect in ((1, dict(reason=4, rows=10, rounds=1)), (2, dict(reason=0, rows=9, rounds=2))):
        problem, _ = random_problem(np.random.default_rng([seed, 1]), n_cam=3, seen=[4, 3, 3], clutter=0, displace=(1, 8.0))
        out.append(dict(name="outlier_%d" % rounds, problem=problem, options=dict(max_rounds=rounds), expect=expect))
    for kind in ("claimed_distinct", "claimed_higher", "claimed_tie", "detection_tie", "detection_tie_swapped"):
        problem, want = exact_problem(kind)
        out.append(dict(name=kind, problem=problem, options=dict(max_rounds=1), expect=dict(match=want)))
    return out, redraws


def check_expectation(shape, w):
    """what shapes() states about a problem, against the witness's (or anyone's) dict"""
    e = shape["expect"]
    for k in ("reason", "rows", "rounds"):
        if k in e:
            assert w[k] == e[k], (shape["name"], k, w[k], e[k])
    if "match" in e:
        assert np.array_equal(w["match"], e["match"]), (shape["name"], w["match"])
    if "behind" in e:
        assert not w["match"][e["behind"]].any() and len(shape["problem"][2][e["behind"]]) > 0, shape["name"]


# ---- the scenario of the GPU tier: a body that is half occluded for every camera ------------------------------------

def rig_cameras(n):
    """n cameras of C2's image size on a 12 cm base line, turned a few degrees towards each other; camera 0 is the rig
    frame (the rig of tests/test_rig_fusion.py)."""
    from rpg_monocular_pose_estimator_amd import synth
    K0, D0 = synth.camera_for(480, 752)
    cams, E = [], []
    for c in range(n):
        K = K0.copy()
        K[0, 0] *= 1.0 + 0.02 * c
        K[1, 1] *= 1.0 - 0.015 * c
        K[0, 2] += 3.0 * c
        cams.append((K, D0 * (1.0 - 0.1 * c)))
        T = np.eye(4)
        if c:
            T[:3, :3] = synth.rodrigues([0.1, 1.0, 0.05 * c], 0.04 * c * (-1) ** c)
            T[:3, 3] = [0.06 * c * (-1) ** c, 0.01 * c, 0.005 * c]
        E.append(T)
    return cams, np.array(E)


SCENARIO = dict(seed=6, frames=14, full=5, partial={0: (0, 1, 2), 1: (2, 3, 4), 2: (0, 4)})


def scenario_sequence(visible=True):
    """3 cameras, C2, SCENARIO["frames"] frames: all LEDs on the first SCENARIO["full"] frames, then camera 0 sees LEDs
    {0, 1, 2}, camera 1 {2, 3, 4} and camera 2 {0, 4} — eight measurements of one pose, no camera with four.
    -> (sequence dict of synth.make_rig_sequence, cams, E)"""
    from rpg_monocular_pose_estimator_amd import synth
    cams, E = rig_cameras(3)
    S = SCENARIO
    vis = {c: {k: ms for k in range(S["full"], S["frames"])} for c, ms in S["partial"].items()} if visible else None
    return synth.make_rig_sequence("C2", S["frames"], S["seed"], cams, E, visible=vis), cams, E


def mixed_batch(n=67, seed=77):
    """n problems over ONE rig (cameras 0 .. 3 the exact camera four times, two drawn ones), ONE marker set (m0 = 0, m1 =
    (1/4, 0, 0), four drawn ones) and the options max_rounds = 1, min_markers = 2, with every way to end interleaved.
    k % 6 == 1: three rows (reason 1); 2: four rows on one marker (reason 2); 3: m0 and m1 on the line y = 0, z = 1 of two
    identical cameras — for every row the Jacobian's column of the y translation is minus that of the x rotation, the
    fourth pivot of the unpivoted LDL^T is an exact 0 and the pose not finite (reason 3); 4: a detection 7 px off its LED
    (reason 4 after the one round, where it was matched); else a good problem.
    -> (cameras, markers, tol_match, tol_accept, options, list of (dets, T_pred), kinds)"""
    rng = np.random.default_rng(seed)
    cameras = [exact_camera() for _ in range(4)] + witness_rig.random_cameras(rng, 2)
    markers = np.vstack([[0, 0, 0], [0.25, 0, 0], rng.uniform(-0.25, 0.25, (4, 3))])
    rig = (cameras, markers)
    options = dict(max_rounds=1, min_rows=4, min_markers=2)
    items, kinds = [], []
    for k in range(n):
        kind = {1: 1, 2: 2, 3: 3, 4: 4}.get(k % 6, 0)
        if kind == 3:
            dets = [np.array([[376.5, 240.0], [476.0, 240.5]])] * 2 + [np.zeros((0, 2))] * 4
            T_pred = np.eye(4)
            T_pred[2, 3] = 1.0
        else:
            kw = {0: dict(seen=[int(rng.integers(2, 7)) for _ in range(6)]), 1: dict(seen=[2, 0, 1, 0, 0, 0], clutter=0),
                  2: dict(seen=[[2], [2], [2], [2], [], []], clutter=0),
                  4: dict(seen=[4, 3, 3, 0, 2, 2], clutter=0, displace=(1, 7.0))}[kind]
            (_, _, dets, T_pred, _, _), _ = random_problem(rng, rig=rig, **kw)
        items.append((dets, T_pred))
        kinds.append(kind)
    return cameras, markers, np.full(6, 12.0), np.full(6, 3.0), options, items, kinds
