"""A numpy witness of the rig initialiser (include/mpe.h, mpe_rig_init_batch), written in ANOTHER formulation than the
device code: the items by nested loops in item order instead of unranking, witness_pipeline.p3p (complex Ferrari through
Python's cmath) for the hypotheses, T_h by 4x4 matrix products with np.linalg.inv, the score of ALL hypotheses at once
from dense distance arrays (hypothesis x marker x detection) with np.argmin, the one-marker-per-detection rule as a
pairwise comparison array, witness_rig_track.rig_track for the tracking rounds.

Knife edges, measured on the witness's OWN numbers (KnifeEdge; the generators re-draw and count):
  * a hypothesis whose row set differs between the tolerance - 1e-6 and + 1e-6 AND whose larger count reaches the
    runner-up's (and is a row at all); other hypotheses decide nothing;
  * the winner and the best key with as many rows and another row set have s2 within 1e-9 relative (or both below
    1e-12 px^2: sums of rounding residue).  A problem whose only camera with three detections has exactly three, or
    clutter alone, is such a problem by nature — every permutation's
    hypotheses pass through the three points —; with allow_tie the witness goes on and marks its dict tie = True, and
    check_against_witness then compares only what does not depend on which of the tied keys won;
  * whatever witness_rig_track.match_round raises at the winner's pose (two detections or two markers as near), and the
    tracking rounds' own.
The count of FINITE solutions is not pinned against this witness (Ferrari's unstable corner may differ between the two
quartics); the item count is."""
import itertools
import json
import os

import numpy as np

import witness_pipeline as WP
import witness_rig
import witness_rig_track as W
from witness_rig_track import KnifeEdge

MARGIN = 1e-6
DEFAULTS = dict(max_rounds=2, min_rows=6, min_markers=4, min_margin=1)


def n_items(dets, n_mk):
    perms = n_mk * (n_mk - 1) * (n_mk - 2) if n_mk >= 3 else 0
    return sum(len(d) * (len(d) - 1) * (len(d) - 2) // 6 * perms for d in dets if len(d) >= 3)


def item_of(dets, n_mk, camera, detection, marker):
    """the item number of (camera, detection triple i < j < k, ordered marker triple), counted in item order"""
    item = n_items(dets[:camera], n_mk)
    perms = list(itertools.permutations(range(n_mk), 3))
    combos = list(itertools.combinations(range(len(dets[camera])), 3))
    return item + combos.index(tuple(detection)) * len(perms) + perms.index(tuple(marker))


def hypotheses(cameras, markers, dets):
    """-> (h (H) int, T (H, 4, 4), what (H) of (camera, detection triple, marker triple, root)) of the finite solutions"""
    markers = np.asarray(markers, float)
    n_mk = len(markers)
    hs, Ts, what = [], [], []
    item = 0
    for c, (K, E) in enumerate(cameras):
        det = np.asarray(dets[c], float).reshape(-1, 2)
        if len(det) < 3 or n_mk < 3:
            continue
        K = np.asarray(K, float).reshape(3, 3)
        Einv = np.linalg.inv(np.asarray(E, float).reshape(4, 4))
        rays = np.stack([(det[:, 0] - K[0, 2]) / K[0, 0], (det[:, 1] - K[1, 2]) / K[1, 1], np.ones(len(det))], axis=1)
        rays /= np.linalg.norm(rays, axis=1)[:, None]
        for tri in itertools.combinations(range(len(det)), 3):       # lexicographic i < j < k
            for perm in itertools.permutations(range(n_mk), 3):      # lexicographic ordered triples of distinct markers
                sols = WP.p3p(rays[list(tri)], markers[list(perm)])
                if sols is not None:
                    for root, (R, Cc) in enumerate(sols):
                        if np.isfinite(R).all() and np.isfinite(Cc).all():
                            H = np.eye(4)                            # marker <- camera
                            H[:3, :3], H[:3, 3] = R, Cc
                            hs.append(4 * item + root)
                            Ts.append(Einv @ np.linalg.inv(H))
                            what.append((c, tri, perm, root))
                item += 1
    assert item == n_items([np.asarray(d).reshape(-1, 2) for d in dets], n_mk)
    return np.array(hs, np.int64), np.array(Ts, float).reshape(-1, 4, 4), what


def score(cameras, markers, dets, tol, Ts):
    """The row sets of all poses Ts at the tolerances tol (n_cam) -> (match (H, n_cam, n_mk) int, 1-based or 0, s2 (H))"""
    markers = np.asarray(markers, float)
    H, n_cam, n_mk = len(Ts), len(cameras), len(markers)
    match = np.zeros((H, n_cam, n_mk), np.int64)
    s2 = np.zeros(H)
    P = np.hstack([markers, np.ones((n_mk, 1))]).T
    for c, (K, E) in enumerate(cameras):
        det = np.asarray(dets[c], float).reshape(-1, 2)
        if len(det) == 0 or H == 0:
            continue
        q = (np.asarray(E, float).reshape(4, 4) @ Ts @ P)[:, :3]                 # (H, 3, n_mk)
        with np.errstate(all="ignore"):
            h = np.asarray(K, float).reshape(3, 3) @ q
            uv = np.swapaxes(h[:, :2] / h[:, 2:3], 1, 2)                         # (H, n_mk, 2)
            vis = (q[:, 2] > 0) & np.isfinite(uv).all(axis=2)
            D = np.sqrt(((np.where(vis[:, :, None], uv, 0.0)[:, :, None, :] - det[None, None]) ** 2).sum(axis=3))
        j = D.argmin(axis=2)                                                     # (H, n_mk): the first minimum
        d = np.take_along_axis(D, j[:, :, None], axis=2)[:, :, 0]
        cand = vis & (d <= tol[c])
        m = np.arange(n_mk)
        # marker a loses to marker b on the same detection that is nearer, or as near and lower
        loses = (cand[:, None, :] & (j[:, :, None] == j[:, None, :]) & (m[None, :, None] != m[None, None, :])
                 & ((d[:, None, :] < d[:, :, None]) | ((d[:, None, :] == d[:, :, None]) & (m[None, None, :] < m[None, :, None]))))
        keep = cand & ~loses.any(axis=2)
        match[:, c, :] = np.where(keep, j + 1, 0)
        s2 += np.where(keep, d * d, 0.0).sum(axis=1)
    return match, s2


def _order(rows, s2, hs):
    return np.lexsort((hs, s2, -rows))  # rows descending, s2 ascending, h ascending


def rig_init(cameras, markers, dets, tol_vote, tol_accept, margin=MARGIN, allow_tie=False, **options):
    """-> dict(status, reason, T, cov, iterations, match, n_items, h, camera, detection, marker, root, best_rows, best_sum2,
    best_markers, runner_rows, T_hyp, n_finite, track: witness_rig_track.rig_track's dict or None)"""
    opt = dict(DEFAULTS, **options)
    markers = np.asarray(markers, float)
    dets = [np.asarray(d, float).reshape(-1, 2) for d in dets]
    n_cam, n_mk = len(cameras), len(markers)
    tol_vote, tol_accept = np.asarray(tol_vote, float), np.asarray(tol_accept, float)
    out = dict(status=1, reason=6, T=np.eye(4), cov=np.zeros((6, 6)), iterations=0, match=np.zeros((n_cam, n_mk), np.int64),
               n_items=n_items(dets, n_mk), h=-1, camera=-1, detection=(-1,) * 3, marker=(-1,) * 3, root=-1, best_rows=0,
               best_sum2=0.0, best_markers=0, runner_rows=0, T_hyp=np.eye(4), n_finite=0, track=None, tie=False)
    hs, Ts, what = hypotheses(cameras, markers, dets)
    out["n_finite"] = len(hs)
    if len(hs) == 0:
        return out
    match, s2 = score(cameras, markers, dets, tol_vote, Ts)
    rows = (match != 0).sum(axis=(1, 2))
    order = _order(rows, s2, hs)
    w = order[0]
    contra = ((match != 0) & (match != match[w][None])).any(axis=(1, 2))
    runner = int(rows[contra].max()) if contra.any() else 0
    # knife edges
    lo, _ = score(cameras, markers, dets, tol_vote - margin, Ts)
    hi, _ = score(cameras, markers, dets, tol_vote + margin, Ts)
    unstable = (lo != hi).any(axis=(1, 2))
    larger = np.maximum((lo != 0).sum(axis=(1, 2)), (hi != 0).sum(axis=(1, 2)))
    if (unstable & (larger >= max(runner, 1))).any():
        raise KnifeEdge("a hypothesis with %d rows at the vote tolerance" % int(larger[unstable].max()))
    rival = (rows == rows[w]) & (match != match[w][None]).any(axis=(1, 2))   # as many rows, another row set
    if rival.any():
        best = s2[rival].min()
        if abs(best - s2[w]) <= 1e-9 * max(best, s2[w]) + 1e-12:
            if not allow_tie:
                raise KnifeEdge("the two best row sets as good")
            out["tie"] = True
    if not np.array_equal(W.match_round(cameras, Ts[w], markers, dets, tol_vote, margin), match[w]):
        raise AssertionError("the witness's two scorings disagree")
    c, tri, perm, root = what[w]
    out.update(reason=0, match=match[w].copy(), h=int(hs[w]), camera=c, detection=tuple(tri), marker=tuple(perm), root=root,
               best_rows=int(rows[w]), best_sum2=float(s2[w]), best_markers=int((match[w] != 0).any(axis=0).sum()),
               runner_rows=runner, T_hyp=Ts[w].copy())
    if out["best_rows"] < opt["min_rows"]:
        out["reason"] = 1
    elif out["best_markers"] < opt["min_markers"]:
        out["reason"] = 2
    elif out["best_rows"] - runner < opt["min_margin"]:
        out["reason"] = 5
    else:
        t = W.rig_track(cameras, markers, dets, Ts[w], tol_vote, tol_accept, max_rounds=opt["max_rounds"],
                        min_rows=opt["min_rows"], min_markers=opt["min_markers"], margin=margin)
        out.update(track=t, reason=t["reason"], match=t["match"], iterations=t["iterations"])
        if t["reason"] == 0:
            out.update(status=0, T=t["T"], cov=t["cov"])
    return out


def check_against_witness(rec, match, info, problem, options=None, what=None, w=None):
    """rec [RESULT_DTYPE], match (n_cam, n_mk), info [RIG_INIT_INFO_DTYPE] of one problem (cameras, markers, dets, tol_vote,
    tol_accept) against the witness: EQUAL reason, item count, winner, best_rows, best_markers, runner_rows, match, and the
    tracking rounds' rounds / rows / distinct markers; T_hyp within 1e-9; the record with witness_rig_track's criteria
    (pose 1e-9, covariance rtol 1e-5 / atol 1e-12, iterations +-1, residuals 1e-6); T = I, cov = 0 without a pose.
    -> the witness's dict."""
    if w is None:
        w = rig_init(*problem, **(options or {}))
    assert int(info["n_items"]) == w["n_items"], (what, int(info["n_items"]), w["n_items"])
    assert int(info["reason"]) == w["reason"], (what, int(info["reason"]), w["reason"], info, w["best_rows"], w["runner_rows"])
    if w["tie"]:  # (only what every one of the tied keys gives: they have the winner's rows, and no pose comes of them)
        assert w["reason"] in (1, 5) and int(info["best_rows"]) == w["best_rows"] and int(rec["n_corr"]) == w["best_rows"], what
        assert int(rec["status"]) == 1 and np.array_equal(rec["T"].reshape(4, 4), np.eye(4)) and not rec["cov"].any(), what
        return w
    got = (int(info["camera"]), tuple(int(x) for x in info["detection"]), tuple(int(x) for x in info["marker"]), int(info["root"]))
    assert got == (w["camera"], w["detection"], w["marker"], w["root"]), (what, got, w["camera"], w["detection"], w["marker"], w["root"])
    assert (int(info["best_rows"]), int(info["best_markers"]), int(info["runner_rows"])) == \
        (w["best_rows"], w["best_markers"], w["runner_rows"]), (what, info, w["best_rows"], w["best_markers"], w["runner_rows"])
    assert np.abs(np.asarray(info["T_hyp"]).reshape(4, 4) - w["T_hyp"]).max() <= 1e-9, what
    assert abs(float(info["best_sum2"]) - w["best_sum2"]) <= 1e-6 * max(1.0, w["best_sum2"]), what
    assert np.array_equal(np.asarray(match).reshape(w["match"].shape), w["match"]), (what, match, w["match"])
    assert int(rec["status"]) == w["status"], what
    assert int(rec["n_corr"]) == int((w["match"] != 0).sum()) and int(rec["n_det"]) == int((w["match"] != 0).any(axis=1).sum()), what
    assert abs(int(rec["gn_iterations"]) - w["iterations"]) <= 1, what
    assert np.abs(rec["T"].reshape(4, 4) - w["T"]).max() <= 1e-9, (what, np.abs(rec["T"].reshape(4, 4) - w["T"]).max())
    assert np.allclose(rec["cov"].reshape(6, 6), w["cov"], rtol=1e-5, atol=1e-12), what
    if w["status"] != 0:
        assert np.array_equal(rec["T"].reshape(4, 4), np.eye(4)) and not rec["cov"].any(), what
    ti, t = info["track"], w["track"]
    if t is None:
        assert not np.frombuffer(np.asarray(ti).tobytes(), np.uint8).any(), (what, ti)
    else:
        assert (int(ti["rounds"]), int(ti["rows"]), int(ti["distinct_markers"]), int(ti["reason"])) == \
            (t["rounds"], t["rows"], t["distinct_markers"], t["reason"]), (what, ti, t)
        if t["reason"] in (0, 4):
            assert abs(float(ti["max_residual"]) - t["max_residual"]) <= 1e-6 and abs(float(ti["rms"]) - t["rms"]) <= 1e-6, what
        else:
            assert float(ti["max_residual"]) == 0.0 and float(ti["rms"]) == 0.0, what
    return w


# ---- problems: (cameras, markers, dets, tol_vote, tol_accept) -------------------------------------------------------

KINDS = ([3, 3, 2], [3, 2, 2], [3, 2, 1], [4, 3, 0])


def random_problem(rng, seen, clutter=2, tol=3.0, **kw):
    """witness_rig_track.random_problem (5 markers, 0.1 px noise, the list shuffled) without its predicted pose; camera c
    sees seen[c] LEDs among `clutter` stray detections; seen = None: the body is absent, 5 stray detections per camera.
    -> (problem, T_true)"""
    if seen is None:
        seen, clutter = [0, 0, 0], 5
    (cameras, markers, dets, _, _, _), T_true = W.random_problem(rng, n_cam=kw.pop("n_cam", len(seen)), seen=seen,
                                                                 clutter=clutter, **kw)
    n = len(cameras)
    return (cameras, markers, dets, np.full(n, float(tol)), np.full(n, float(tol))), T_true


def draw(key, seen, options=None, attempt=None, allow_tie=False, **kw):
    """random_problem from the generator seeded with key + [attempt]; attempt = None: 0, 1, .. until the witness meets no
    knife edge -> (problem, T_true, witness dict, attempt); attempt given (a recorded one): that draw, no witness run ->
    (problem, T_true, None, attempt)"""
    if attempt is not None:
        problem, T_true = random_problem(np.random.default_rng(list(key) + [attempt]), seen, **kw)
        return problem, T_true, None, attempt
    for attempt in range(20):
        problem, T_true = random_problem(np.random.default_rng(list(key) + [attempt]), seen, **kw)
        try:
            return problem, T_true, rig_init(*problem, allow_tie=allow_tie, **(options or {})), attempt
        except KnifeEdge:
            pass
    raise AssertionError("the generator keeps meeting knife edges")


DRAW_SEED = 2026
SHAPE_SEED = 20261020
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rig_init_witness.json")
_TRACK_KEYS = ("rounds", "rows", "distinct_markers", "reason", "max_residual", "rms")


def pack(w, attempt):
    """a witness dict as JSON holds it (of the tracking rounds only what check_against_witness reads)"""
    d = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in w.items() if k != "track"}
    d["track"] = None if w["track"] is None else {k: w["track"][k] for k in _TRACK_KEYS}
    d["attempt"] = attempt
    return d


def unpack(d):
    w = dict(d)
    for k, shape in (("T", (4, 4)), ("cov", (6, 6)), ("T_hyp", (4, 4))):
        w[k] = np.array(d[k], float).reshape(shape)
    w["match"] = np.array(d["match"], np.int64)
    w["detection"], w["marker"] = tuple(d["detection"]), tuple(d["marker"])
    return w


def recorded():
    """tests/golden/rig_init_witness.json: the witness's dicts of drawn_problems() and shapes(), written by `python
    tests/witness_rig_init.py --record` and compared with a fresh run by the CPU tier (tests/test_rig_init_host.py) — so that
    the GPU tier need not run the Python P3P over 150 000 items again"""
    with open(GOLDEN) as fh:
        return json.load(fh)


def same_witness(a, b):
    """two witness dicts (one may come from the record): integers equal, floats within 1e-10"""
    for k in ("status", "reason", "iterations", "n_items", "h", "camera", "root", "best_rows", "best_markers", "runner_rows", "tie"):
        if a[k] != b[k]:
            return False
    if tuple(a["detection"]) != tuple(b["detection"]) or tuple(a["marker"]) != tuple(b["marker"]):
        return False
    if not np.array_equal(a["match"], b["match"]) or (a["track"] is None) != (b["track"] is None):
        return False
    for k in ("T", "cov", "T_hyp"):
        if not np.allclose(a[k], b[k], rtol=0, atol=1e-10):
            return False
    if abs(a["best_sum2"] - b["best_sum2"]) > 1e-10:
        return False
    return a["track"] is None or all(abs(a["track"][k] - b["track"][k]) <= 1e-10 for k in _TRACK_KEYS)


def drawn_problems(n_body=60, n_absent=20, seed=DRAW_SEED, record=None):
    """n_body problems of the kinds [3, 3, 2], [3, 2, 2], [3, 2, 1], [4, 3, 0] in turn, then n_absent with the body absent.
    record: recorded()["drawn"] — the problems are drawn as recorded and the witness is not run.
    -> (list of dict(kind, problem, T_true, w, attempt), re-draws)"""
    out, redraws = [], 0
    for k in range(n_body + n_absent):
        seen = KINDS[k % len(KINDS)] if k < n_body else None
        if record is None:
            # (clutter alone: the best hypotheses are those through three detections, tied at s2 = rounding residue)
            problem, T_true, w, attempt = draw([seed, k], seen, allow_tie=seen is None)
        else:
            problem, T_true, _, attempt = draw([seed, k], seen, attempt=record[k]["attempt"])
            w = unpack(record[k])
        redraws += attempt
        out.append(dict(kind=seen, problem=problem, T_true=T_true, w=w, attempt=attempt))
    return out, redraws


def nearly_symmetric_markers():
    """four markers on a square of 0.2 m, each a few millimetres off it: the quarter turn about z maps the set onto itself
    to within a pixel at 1.5 m, so a wrong assignment explains every row within 3 px — with another s2"""
    return np.array([[0.1, 0.1, 0.0], [-0.1, 0.103, 0.004], [-0.097, -0.1, -0.003], [0.1, -0.104, 0.002]])


def shapes(seed=SHAPE_SEED, record=None):
    """The exact shapes of the issue but the list of 64 (long_list below: too many items for this witness).  record:
    recorded()["shapes"], as drawn_problems takes it.
    -> (list of dict(name, problem, options, expect: what the WITNESS must say, w, attempt), re-draws)"""
    out = []
    rigs = np.random.default_rng([seed, 99])
    line = np.array([[0.0, 0, 0], [0.1, 0, 0], [0.2, 0, 0], [0.05, 0.2, 0.05], [-0.1, 0.1, 0.15]])
    line_rig = (witness_rig.random_cameras(rigs, 2), line)
    sym_rig = (witness_rig.random_cameras(rigs, 2), nearly_symmetric_markers())

    def add(name, seen, options, expect, allow_tie=False, same_as=None, **kw):
        k = len(out)
        if same_as is not None:  # the problem of an earlier shape under other options
            problem, attempt = out[same_as]["problem"], out[same_as]["attempt"]
            w = rig_init(*problem, **options) if record is None else unpack(record[k])
        elif record is not None:
            problem, _, _, attempt = draw([seed, k], seen, attempt=record[k]["attempt"], **kw)
            w = unpack(record[k])
        else:
            problem, _, w, attempt = draw([seed, k], seen, options, allow_tie=allow_tie, **kw)
        out.append(dict(name=name, problem=problem, options=options, expect=expect, w=w, attempt=attempt))

    add("one_camera_three", [3], {}, dict(reason=1, best_rows=3, n_items=60, tie=True), allow_tie=True, clutter=0)
    # camera 0 sees the collinear triple {0, 1, 2}, camera 1 two others: the true permutations have no hypothesis
    add("collinear", [[0, 1, 2], [3, 4]], {}, dict(collinear=True, n_items=60, reason=1, best_rows=3, tie=True), allow_tie=True,
        clutter=0, rig=line_rig)
    add("tie", [4, 4], {}, dict(reason=5, best_rows=8, runner_rows=8), clutter=0, rig=sym_rig)
    add("tie_no_margin", None, dict(min_margin=0), dict(reason=0, best_rows=8, runner_rows=8), same_as=2)
    add("behind", [3, 3, 3], {}, dict(behind=2), backwards=2, clutter=1)
    add("three_markers", [3, 3], {}, dict(reason=2, best_rows=6, n_items=12), n_mk=3, clutter=0)
    add("three_markers_allowed", None, dict(min_markers=3), dict(best_rows=6, n_items=12), same_as=5)
    add("sixteen_by_two", [2] * 16, {}, dict(reason=6, n_items=0), clutter=0)
    return out, sum(s["attempt"] for s in out)


def check_expectation(shape, w):
    e = shape["expect"]
    for k in ("reason", "best_rows", "runner_rows", "n_items"):
        if k in e:
            assert w[k] == e[k], (shape["name"], k, w[k], e[k])
    assert w["tie"] == e.get("tie", False), shape["name"]
    if "behind" in e:  # the camera has detections and hypotheses of its own, and no row
        assert len(shape["problem"][2][e["behind"]]) >= 3 and not w["match"][e["behind"]].any(), shape["name"]
    if "collinear" in e:
        assert w["camera"] in (0, -1) and sorted(w["marker"]) != [0, 1, 2], shape["name"]


def long_list(seed=7):
    """One camera with 64 detections — four exact pixels of the four markers at the END of the list, 60 stray ones in
    front — and 4 markers: 41 664 x 24 = 999 936 items, the winner in the last block of the 7 812.  Too many for this
    witness's Python P3P; what must come out is known by construction: the first hypothesis in item order that explains
    all four LEDs exactly, from the detection triple (60, 61, 62) with the markers (0, 1, 2).
    -> (problem, expected dict(n_items, camera, detection, marker, item, best_rows, T_true))"""
    rng = np.random.default_rng(seed)
    cameras = [W.exact_camera()]
    markers = np.array([[-0.25, -0.125, 0.0], [0.25, -0.125, 0.05], [0.25, 0.125, 0.0], [-0.25, 0.125, 0.1]])
    T_true = witness_rig._rigid(rng, 0.3, [0.05, -0.02, 1.5])
    uv, _ = W.project(cameras, T_true, markers)
    stray = []
    while len(stray) < 60:
        p = np.array([rng.uniform(0, 752), rng.uniform(0, 480)])
        if np.linalg.norm(uv[0] - p, axis=1).min() > 40.0:
            stray.append(p)
    dets = [np.vstack([np.array(stray), uv[0]])]
    problem = (cameras, markers, dets, np.array([3.0]), np.array([3.0]))
    item = item_of(dets, 4, 0, (60, 61, 62), (0, 1, 2))
    return problem, dict(n_items=n_items(dets, 4), camera=0, detection=(60, 61, 62), marker=(0, 1, 2), item=item, best_rows=4,
                         T_true=T_true)


def check_long_list(rec, match, info, expect):
    """what the list of 64 must give, by construction (witness_rig_init.long_list)"""
    assert int(info["n_items"]) == expect["n_items"] == 999936
    assert int(info["reason"]) == 1 and int(info["best_rows"]) == 4 and int(info["best_markers"]) == 4 and rec["status"] == 1
    # one of the four triples of the detections 60 .. 63 with their own markers; the first of them is in the LAST block
    d, m = tuple(int(x) for x in info["detection"]), tuple(int(x) for x in info["marker"])
    assert int(info["camera"]) == 0 and min(d) >= 60 and tuple(x - 60 for x in d) == m, (d, m)
    assert expect["item"] // 128 == (expect["n_items"] - 1) // 128
    assert np.array_equal(np.asarray(match).reshape(1, 4), [[61, 62, 63, 64]])
    assert float(info["best_sum2"]) < 1e-12 and np.abs(np.asarray(info["T_hyp"]).reshape(4, 4) - expect["T_true"]).max() < 1e-6
    assert np.array_equal(rec["T"].reshape(4, 4), np.eye(4)) and not rec["cov"].any()


# ---- the scenario of the GPU tier: the body partly hidden from EVERY camera from frame 0 on --------------------------

SCENARIO = dict(seed=6, frames=10, partial={0: (0, 1, 2), 1: (2, 3, 4), 2: (0, 4)})


def scenario_sequence(blank=()):
    """3 cameras, C2, 10 frames; on every frame camera 0 sees the LEDs {0, 1, 2}, camera 1 {2, 3, 4}, camera 2 {0, 4};
    on the frames `blank` no camera sees any.  -> (sequence dict of synth.make_rig_sequence, cams, E)"""
    from rpg_monocular_pose_estimator_amd import synth
    cams, E = W.rig_cameras(3)
    S = SCENARIO
    vis = {c: {k: (() if k in blank else ms) for k in range(S["frames"])} for c, ms in S["partial"].items()}
    return synth.make_rig_sequence("C2", S["frames"], S["seed"], cams, E, visible=vis), cams, E


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["--record"]:
        drawn, _ = drawn_problems()
        shaped, _ = shapes()
        with open(GOLDEN, "w") as fh:
            json.dump(dict(drawn=[pack(p["w"], p["attempt"]) for p in drawn], shapes=[pack(s["w"], s["attempt"]) for s in shaped]), fh)
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
