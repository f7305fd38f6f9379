"""Several bodies in one frame on the device (mpe_rig_init_bodies_batch: the peel kernels of mpe_rig_peel.hip around the rig
initialiser's launches; mpe_rig_init_bodies_trackers; Bodies.step).  The yardstick is the parent's entry: every (problem,
body) record, info and match equals, byte for byte with the indices translated, what rig_init_batch returns for the lists
THIS file filtered on the host with that body's markers and options.  Besides: the recorded witness
(tests/golden/rig_bodies_witness.json, which the CPU tier holds against a fresh run), a record does not depend on its
batch, one submission per call, and two identical bodies in front of one camera followed through a rendered sequence."""
import numpy as np
import pytest

import rpg_monocular_pose_estimator_amd as mpe
from rpg_monocular_pose_estimator_amd import synth
import witness_rig
import witness_rig_bodies as WB
from test_rig_bodies_host import check_rounds_against_single

pytestmark = pytest.mark.gpu


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def dev_bodies(hip, problem):
    """-> (records (n_bodies), match (n_bodies, n_cam, MAX_MARKERS), info (n_bodies), owner per camera) of one problem"""
    rec, match, info, owner = hip.rig_init_bodies_batch(
        problem["cameras"], problem["bodies"], [problem["dets"]], problem["tol_vote"], problem["tol_accept"],
        claimed=None if problem.get("claimed") is None else [problem["claimed"]],
        find=None if problem.get("find") is None else [problem["find"]])
    return rec[0], match[0], info[0], owner[0]


def parent(hip, problem):
    """the parent's entry over lists filtered on the host: (markers, lists, options) -> (record, match, info)"""
    def run(markers, lists, options):
        rec, match, info = hip.rig_init_batch(problem["cameras"], markers, [lists], problem["tol_vote"], problem["tol_accept"], **options)
        return rec[0], match[0], info[0]
    return run


@pytest.fixture(scope="module")
def problems():
    """the exact shapes and the drawn problems with the recorded witness answers (the witness is not run here)"""
    record = WB.recorded()
    shapes, _ = WB.shapes(record=record["shapes"])
    drawn, _ = WB.drawn_problems(record=record["drawn"])
    return shapes, drawn


def test_drawn_problems_and_shapes_against_the_parents_entry_and_the_witness(hip, problems):
    shapes, drawn = problems
    assert len(drawn) == 60 and [s["name"] for s in shapes] == [name for name, _ in WB.SHAPES]
    for k, p in enumerate(shapes + drawn):
        what = p.get("name", k)
        got = dev_bodies(hip, p["problem"])
        check_rounds_against_single(p["problem"], got, parent(hip, p["problem"]), what)
        WB.check_against_witness(*got, p["problem"], what, ws=p["ws"])
    for s in shapes:
        WB.check_expectation(s)


def test_the_full_range_of_bodies_against_the_parents_entry(hip):
    """1 - 4 bodies out of {M4, M5, M5, M8} with M8 in full view, no item budget and no witness: every round against
    rig_init_batch over the lists filtered here"""
    problems = WB.parity_problems()
    n_bodies, m8_found, fourth_found = {}, 0, 0
    for k, p in enumerate(problems):
        pr = p["problem"]
        got = dev_bodies(hip, pr)
        check_rounds_against_single(pr, got, parent(hip, pr), k)
        n_bodies[len(pr["bodies"])] = n_bodies.get(len(pr["bodies"]), 0) + 1
        m8_found += sum(int(i["reason"]) == 0 and len(M) == 8 for i, (M, _) in zip(got[2], pr["bodies"]))
        fourth_found += int(len(pr["bodies"]) == 4 and int(got[2][3]["reason"]) == 0)
    assert set(n_bodies) == {1, 2, 3, 4} and n_bodies[4] >= 8 and m8_found >= 8 and fourth_found >= 3, (n_bodies, m8_found, fourth_found)


def test_a_list_of_64_with_both_ends_claimed(hip):
    """62 free points x 4 markers = 907 680 items in 7 092 blocks, counted from the 62 the claims leave"""
    made = WB.claimed_ends()
    got = dev_bodies(hip, made[0])
    WB.check_claimed_ends(*got, made)
    check_rounds_against_single(made[0], got, parent(hip, made[0]), "claimed_ends")


def test_the_bodies_in_reverse_order(hip, problems):
    s = [x for x in problems[0] if x["name"] == "identical"][0]
    a, b = dev_bodies(hip, s["problem"]), dev_bodies(hip, WB.reversed_problem(s["problem"]))
    assert all(_same(x, y) for x, y in zip(a[:3], b[:3])) and _same(a[3][0], b[3][0])  # (round k owns the same points)
    made = WB._one_camera(np.random.default_rng([WB.SHAPE_SEED, 65]), ["M5", "M4"], strays=2)
    for pr in (made[0], WB.reversed_problem(made[0])):
        check_rounds_against_single(pr, dev_bodies(hip, pr), parent(hip, pr), pr["names"])


def test_one_body_without_claims_is_rig_init_batch(hip, problems):
    n = 0
    for k, p in enumerate(problems[1]):
        pr = p["problem"]
        if len(pr["bodies"]) != 1:
            continue
        M = pr["bodies"][0][0]
        rec, match, info, owner = dev_bodies(hip, pr)
        r, m, i = hip.rig_init_batch(pr["cameras"], M, [pr["dets"]], pr["tol_vote"], pr["tol_accept"], **WB.body_options(pr, 0))
        assert _same(rec[0], r[0]) and _same(info[0], i[0]) and _same(match[0][:, :len(M)], m[0]) and not match[0][:, len(M):].any(), k
        n += 1
    assert n >= 10, n


def mixed_batch(n=130, seed=130):
    """n problems over ONE rig of 16 cameras and two M5 bodies, in turn: both bodies in full view of camera 0 and two LEDs
    of each in camera 1 (body 0 found); three LEDs of one body and a stray point (body 0 not found); nothing in view; every camera with three points,
    the even ones of body 0 and the odd ones of body 1"""
    rng = np.random.default_rng(seed)
    cameras = witness_rig.random_cameras(rng, 16, identity_first=True)
    markers = [synth.M5, synth.M5]
    none = [0] * 16
    items = []
    for k in range(n):
        kind = k % 4
        if kind == 0:
            seen, present, strays = [[None, 2] + none[2:], [None, 2] + none[2:]], [True, True], 2  # (seven rows a body)
        elif kind == 1:
            seen, present, strays = [[3] + none[1:], none], [True, False], 1
        elif kind == 2:
            seen, present, strays = [none, none], [False, False], 0
        else:
            seen, present, strays = [[3 if c % 2 == 0 else 0 for c in range(16)], [3 if c % 2 else 0 for c in range(16)]], [True, True], 0
        dets, _, _ = WB.place_bodies(rng, cameras, markers, present, seen=seen, strays=strays)
        items.append(dets)
    return cameras, [(M, None) for M in markers], items


def test_a_record_does_not_depend_on_its_batch(hip):
    cameras, bodies, items = mixed_batch()

    def call(sub):
        return hip.rig_init_bodies_batch(cameras, bodies, sub, 3.0, 3.0)

    alone = [call([d]) for d in items]
    reasons = [tuple(int(r) for r in a[2]["reason"][0]) for a in alone]
    assert {(0, 0), (6, 6)} <= set(reasons) and any(r[0] == 1 for r in reasons), set(reasons)
    assert all(r == (0, 0) for r in reasons[3::4]), reasons[3::4]  # 16 cameras x 3 points: 24 rows a body
    rec, match, info, owner = call(items)
    for k in range(len(items)):
        assert _same(rec[k], alone[k][0][0]) and _same(match[k], alone[k][1][0]) and _same(info[k], alone[k][2][0]), k
        assert all(_same(a, b) for a, b in zip(owner[k], alone[k][3][0])), k
    again = call(items)
    assert _same(again[0], rec) and _same(again[1], match) and _same(again[2], info)
    assert all(_same(a, b) for x, y in zip(again[3], owner) for a, b in zip(x, y))


def test_one_submission_per_call_and_refusals_move_nothing(hip):
    made = WB._one_camera(np.random.default_rng([WB.SHAPE_SEED, 66]), ["M5", "M5", "M4", "M4"], strays=2)
    names = ("rig_init_bodies_submits", "rig_init_submits", "bruteforce_submits")
    before = [hip.get_option(n) for n in names]
    rec, match, info, owner = dev_bodies(hip, made[0])
    assert [hip.get_option(n) for n in names] == [before[0] + 1, before[1], before[2]]
    assert [int(r) for r in info["reason"]] == [0, 0, 0, 0] and np.array_equal(np.where(owner[0] < 0, -1, 0), np.where(made[1][0] < 0, -1, 0))
    bad = dict(made[0], bodies=[(synth.M5, dict(min_rows=2))])
    with pytest.raises(mpe.MpeError, match="min_rows"):
        dev_bodies(hip, bad)
    with pytest.raises(mpe.MpeError, match="MPE_MAX_BODIES"):
        dev_bodies(hip, dict(made[0], bodies=[(synth.M4, None)] * 17))
    six = np.vstack([synth.M5, [[0.1, 0.1, 0.1]]])
    with pytest.raises(mpe.MpeError, match="2\\^22"):
        hip.rig_init_bodies_batch(made[0]["cameras"], [six], [[np.zeros((64, 2))]], 3.0, 3.0)
    assert [hip.get_option(n) for n in names] == [before[0] + 1, before[1], before[2]]
    again = dev_bodies(hip, made[0])  # the handle is usable
    assert all(_same(x, y) for x, y in zip(again[:3], (rec, match, info)))


def test_a_rig_of_two_cameras_and_two_bodies(hip):
    """each camera sees three LEDs of one body and two of the other: no camera could find either on its own"""
    rng = np.random.default_rng([WB.SHAPE_SEED, 67])
    cameras = witness_rig.random_cameras(rng, 2, identity_first=True)
    dets, truth, T_true = WB.place_bodies(rng, cameras, [synth.M5, synth.M5], [True, True],
                                          seen=[[[0, 1, 2], [3, 4]], [[0, 1], [2, 3, 4]]])
    tol = np.full(2, 3.0)
    # (five rows of five markers a body: the rig defaults' six rows are out of reach)
    pr = dict(cameras=cameras, bodies=[(synth.M5, dict(min_rows=5)), (synth.M5, dict(min_rows=5))], dets=dets, tol_vote=tol,
              tol_accept=tol, claimed=None, find=None)
    got = dev_bodies(hip, pr)
    rec, match, info, owner = got
    assert [int(r) for r in info["reason"]] == [0, 0], info["reason"]
    c, m = np.argwhere(match[0] != 0)[0]
    first = int(truth[c][match[0][c, m] - 1])  # the true body that body 0 is
    for b, t in ((0, first), (1, 1 - first)):
        assert np.abs(rec[b]["T"].reshape(4, 4) - T_true[t])[:3, 3].max() < 5e-3
        for c in range(2):
            assert np.array_equal(np.asarray(owner[c]) == b, truth[c] == t)
    check_rounds_against_single(pr, got, parent(hip, pr), "rig")


# ---- two identical bodies in front of one camera, through a rendered sequence ------------------------------------------
# The pose bounds: the same poses rendered with one body at a time (make_bodies_sequence(only=b): the background noise is
# another draw, nothing else differs) through the parent's single Tracker gave, over the 2 x 8 frames, at most
# SINGLE_POS m and SINGLE_ROT rad against the truth (test_the_single_tracker_bounds measures them again and holds them to
# these figures); the bodies' poses may be twice as far off.
SEQ = dict(config="C2", n=8, seed=5, n_bodies=2, min_sep=40.0)
SINGLE_POS = 0.0029529546664585544   # m   (measured on the MI355X: 2.95 mm)
SINGLE_ROT = 0.006880851731037926    # rad (6.88 mrad)


def _errors(T, T_true):
    dR = T[:3, :3].T @ T_true[:3, :3]
    return float(np.linalg.norm(T[:3, 3] - T_true[:3, 3])), float(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))


def _trackers(hip, seq, n):
    return [[mpe.Tracker(hip, seq["markers"][b], seq["K"], seq["D"], mpe.demo_params())] for b in range(n)]


def single_tracker_errors(hip):
    worst = [0.0, 0.0]
    for b in range(SEQ["n_bodies"]):
        seq = synth.make_bodies_sequence(**SEQ, only=b)
        t = mpe.Tracker(hip, seq["markers"][b], seq["K"], seq["D"], mpe.demo_params())
        for k in range(SEQ["n"]):
            r = t.estimate(seq["frames"][k], seq["times"][k])
            assert r["updated"], (b, k)
            e = _errors(r["T"], seq["T_true"][b][k])
            worst = [max(worst[0], e[0]), max(worst[1], e[1])]
        t.close()
    return worst


def test_the_single_tracker_bounds(hip):
    pos, rot = single_tracker_errors(hip)
    print("single tracker, one body at a time: %.6g m, %.6g rad" % (pos, rot))
    assert pos <= SINGLE_POS * 1.0000001 and rot <= SINGLE_ROT * 1.0000001, (pos, rot)


def _run(hip, seq):
    """-> per frame (records, info, owner, last_init, the true body of every body's pose or None, submits so far)"""
    trackers = _trackers(hip, seq, SEQ["n_bodies"])
    bodies = mpe.Bodies(hip, trackers)
    out = []
    for k in range(SEQ["n"]):
        rec, info, owner = bodies.step([seq["frames"][k]], [seq["times"][k]])
        who = []
        for b in range(SEQ["n_bodies"]):
            who.append(None)
            if rec[b]["status"] == 0:
                for t in range(SEQ["n_bodies"]):
                    pos, rot = _errors(rec[b]["T"].reshape(4, 4), seq["T_true"][t][k])
                    if pos <= 2 * SINGLE_POS and rot <= 2 * SINGLE_ROT:
                        who[b] = t
        out.append((rec.copy(), info.copy(), owner, bodies.last_init, who, hip.get_option("rig_init_bodies_submits")))
    for ts in trackers:
        ts[0].close()
    return out


def test_two_identical_bodies_are_found_and_followed(hip):
    seq = synth.make_bodies_sequence(**SEQ)
    before = hip.get_option("rig_init_bodies_submits")
    out = _run(hip, seq)
    rec, info, owner, last_init, who, submits = out[0]
    assert sorted(who) == [0, 1], (who, rec["status"])                     # both bodies, on different true bodies
    assert submits == before + 1 and last_init is not None
    assert len(owner[0]) == 10 and sorted(np.bincount(owner[0] + 1, minlength=3).tolist()) == [0, 5, 5], owner  # five and five
    first = who
    for k in range(1, SEQ["n"]):
        rec, info, owner, last_init, who, submits = out[k]
        assert who == first, (k, who)                                      # each tracker keeps ITS body
        assert submits == before + 1 and last_init is None and owner is None, k   # no initialiser runs
        assert not info[:, :, 7].any(), (k, info[:, :, 7])


def test_a_body_that_is_hidden_comes_back_beside_the_other(hip):
    hidden = 1
    seq = synth.make_bodies_sequence(**SEQ, dropout={hidden: (3, 4)})
    before = hip.get_option("rig_init_bodies_submits")
    out = _run(hip, seq)
    first = out[0][4]
    assert sorted(first) == [0, 1]
    b_hidden = first.index(hidden)
    for k in range(SEQ["n"]):
        rec, info, owner, last_init, who, submits = out[k]
        assert len({w for w in who if w is not None}) == len([w for w in who if w is not None]), (k, who)  # never one body twice
        assert who[1 - b_hidden] == 1 - hidden, (k, who)                   # the body in view is followed throughout
        if k in (3, 4):
            assert who[b_hidden] is None and rec[b_hidden]["status"] != 0, (k, who)
            assert last_init is not None and int(last_init[2][b_hidden]["reason"]) != 0
            assert int(last_init[2][1 - b_hidden]["reason"]) == WB.NOT_ASKED
            assert (owner[0] == -2).sum() == 5 and not (owner[0] >= 0).any(), (k, owner)   # the other's points, claimed by radius
        elif k == 5:                                                       # back in view: found in what the other leaves
            assert who[b_hidden] == hidden and last_init is not None, (k, who)
            assert (owner[0] == -2).sum() == 5 and (owner[0] == b_hidden).sum() == 5, (k, owner)
        else:
            assert who[b_hidden] == hidden, (k, who)
    assert out[-1][5] == before + 4                                        # frames 0, 3, 4 and 5
