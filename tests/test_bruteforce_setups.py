"""Brute-force initialisation of detection sets that differ in camera, marker set and parameters in ONE device
submission (mpe_solve_bruteforce_batch_setups; k2_vote_setups + k3_tail_setups), and the lock-step driver on top of it:
every item must give, byte for byte, what mpe_solve_bruteforce_batch gives the items of its set-up alone.  CPU tier:
export, usage errors, the block table as a stand-alone host program (plain and under sanitizers); GPU tier: the entry
against the parent entry and the oracle, item order, degenerate calls, submission counts, the tracker entries."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from rpg_monocular_pose_estimator_amd import synth
import rpg_monocular_pose_estimator_amd as mpe
from util import pose_diff, POS_TOL_M, ROT_TOL_RAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")
ROWS, COLS = 480, 752


@pytest.fixture(scope="module")
def lib():
    mpe.build_library()
    return mpe.load_library()


def _camera_b():
    K = synth.README_K.copy()
    K[0, 0] *= 1.1
    K[1, 1] *= 1.1
    K[0, 2] += 14.0
    K[1, 2] -= 9.0
    return K, np.array([-0.30, 0.12, 0.0003, -0.0001, 0.0])


def _camera_c():
    K = synth.README_K.copy()
    K[0, 0] *= 0.95
    K[1, 1] *= 0.95
    K[0, 2] -= 11.0
    K[1, 2] += 7.0
    return K, np.array([-0.40, 0.18, -0.0004, 0.0002, -0.01])


def _setup_specs():
    """(markers, K, D, parameter overrides): the 4-LED demo rig with camera a, 5 markers with camera b, 8 markers with
    back-projection tolerance 2 and camera c; a fourth set-up that no item names."""
    Ka, Da = synth.camera_for(ROWS, COLS)
    (Kb, Db), (Kc, Dc) = _camera_b(), _camera_c()
    return [(synth.M4, Ka, Da, {}), (synth.M5, Kb, Db, {}), (synth.M8, Kc, Dc, dict(back_projection_pixel_tolerance=2.0)),
            (synth.M5, Ka, Da, dict(back_projection_pixel_tolerance=3.0))]


def _hip_setups():
    return [(M, K, D, mpe.demo_params(**kw)) for (M, K, D, kw) in _setup_specs()]


# (set-up, detections, marker projections among them): interleaved over the three set-ups; n_det 0, 3, 4, 5, 6, 12, 33
# and 40 — the wide frames (more than 32 detections) on the 4- and 5-marker set-ups —, item 8 distractors only
PLAN = [(0, 4, 4), (1, 5, 5), (2, 12, 8), (0, 0, 0), (1, 3, 3), (2, 6, 6), (0, 33, 4), (1, 40, 5), (2, 5, 0), (0, 6, 4),
        (1, 12, 5), (2, 12, 8), (0, 5, 4), (1, 6, 5)]
SEED = 4129   # (chosen on the CPU with the oracle: every set-up has an item with a pose, and some items have none)


def _items(seed=SEED):
    """Detections of every item of PLAN: projections of the set-up's markers from a seeded pose through the set-up's K
    (undistorted pixels, as findLeds hands them on), seeded distractor points, in seeded order."""
    specs = _setup_specs()
    dets = []
    for i, (s, n_det, n_true) in enumerate(PLAN):
        M, K, D, _ = specs[s]
        rng = np.random.default_rng([seed, i])
        T, spots = synth.sample_scene(rng, M, K, D, ROWS, COLS, n_det - n_true)   # (spots: the LEDs, then the distractors)
        px = synth.project(T, M, K)[np.sort(rng.permutation(len(M))[:n_true])]
        pts = np.vstack([px.reshape(-1, 2), spots[len(M):].reshape(-1, 2)])
        assert len(pts) == n_det
        dets.append(np.ascontiguousarray(pts[rng.permutation(n_det)], np.float64).reshape(-1, 2))
    return dets, [s for (s, _, _) in PLAN]


# ---- CPU tier -----------------------------------------------------------------------------------------------------

def test_entry_is_exported(lib):
    assert "mpe_solve_bruteforce_batch_setups" in mpe.exported_symbols()
    assert hasattr(lib, "mpe_solve_bruteforce_batch_setups")
    assert callable(mpe.Handle.solve_bruteforce_batch) and callable(mpe.Handle.solve_bruteforce_batch_setups)


class _TrackSetup(ctypes.Structure):  # mpe_track_setup
    _fields_ = [("p", ctypes.c_void_p), ("K", ctypes.c_void_p), ("D", ctypes.c_void_p), ("nD", ctypes.c_int),
                ("markers_xyz", ctypes.c_void_p), ("n_markers", ctypes.c_int)]


def test_entry_rejects_bad_usage_without_a_device(lib):
    """Null pointers, set-up indices out of range, marker and detection counts out of range: MPE_ERR_ARG with a null
    handle, before any device work; n == 0 is MPE_OK and looks at no handle."""
    call = lib.mpe_solve_bruteforce_batch_setups
    P = mpe.demo_params()
    K = np.ascontiguousarray(synth.README_K, np.float64)
    M = np.ascontiguousarray(synth.M5, np.float64)
    xy = np.zeros((2, mpe.binding.MAX_DETECTIONS, 2))
    nd = np.array([5, 5], np.int32)
    out = np.zeros(2, mpe.RESULT_DTYPE)

    def setups(n_markers=5, p=ctypes.addressof(P), k=K.ctypes.data, m=M.ctypes.data):
        return (_TrackSetup * 2)(_TrackSetup(p, k, None, 0, m, n_markers), _TrackSetup(p, k, None, 0, m, 5))

    def run(h=None, xy_=xy, nd_=nd, idx=(0, 1), n=2, su=None, n_setups=2, out_=out):
        su = setups() if su is None else su
        return call(h, None if xy_ is None else xy_.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                    None if nd_ is None else nd_.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                    None if idx is None else (ctypes.c_int * len(idx))(*idx), n, su, n_setups,
                    None if out_ is None else ctypes.c_void_p(out_.ctypes.data), None, None)

    assert run() == -1                                   # null handle
    fake = ctypes.create_string_buffer(64)               # a stand-in handle that no refused call looks into
    h = ctypes.addressof(fake)
    assert run(h, n=0) == 0                              # nothing to do
    assert run(h, n=0, idx=None, n_setups=1) == 0
    assert run(None, n=0) == -1
    # everything below is refused before the handle is used: with a null handle
    assert run(None, n=-1) == -1
    assert run(None, xy_=None) == -1 and run(None, nd_=None) == -1 and run(None, out_=None) == -1
    assert call(None, xy.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), nd.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                (ctypes.c_int * 2)(0, 1), 2, None, 2, ctypes.c_void_p(out.ctypes.data), None, None) == -1   # no set-ups
    assert run(None, n_setups=0) == -1
    assert run(None, idx=None) == -1                     # item_setup may be null with one set-up only
    assert run(None, idx=(0, 2)) == -1 and run(None, idx=(-1, 0)) == -1
    assert run(None, su=setups(n_markers=0)) == -1 and run(None, su=setups(n_markers=17)) == -1
    assert run(None, su=setups(p=None)) == -1 and run(None, su=setups(k=None)) == -1 and run(None, su=setups(m=None)) == -1
    assert run(None, nd_=np.array([5, -1], np.int32)) == -1
    assert run(None, nd_=np.array([mpe.binding.MAX_DETECTIONS + 1, 5], np.int32)) == -1


def _build_block_table_program(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC] + flags +
                          [os.path.join(ROOT, "tests", "host", "brute_blocks_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "brute_blocks_host ok: 11 lists" in r.stdout, r.stdout


def test_block_table_on_the_host(tmp_path):
    """csrc/mpe_brute_blocks.h as a stand-alone host program: item lists that mix hypothesis counts 0, 96, 600, 73 920
    and 2.5 M under grid caps that bind — every hypothesis of every item is met by exactly one (block, stride) pair, no
    block names an item that cannot vote, and an item's entries are those of the list that holds it alone."""
    _build_block_table_program(tmp_path, "brute_blocks_host", ["-O2"])


def test_block_table_on_the_host_under_sanitizers(tmp_path):
    _build_block_table_program(tmp_path, "brute_blocks_host_san",
                               ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_items_of_the_plan():
    dets, item_setup = _items()
    assert [len(d) for d in dets] == [n for (_, n, _) in PLAN] and item_setup == [s for (s, _, _) in PLAN]
    assert sorted(set(len(d) for d in dets)) == [0, 3, 4, 5, 6, 12, 33, 40]
    assert set(item_setup) == {0, 1, 2}
    for d in dets:
        assert np.isfinite(d).all()


# ---- GPU tier -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def handle():
    h = mpe.Handle(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def case():
    dets, item_setup = _items()
    return dict(dets=dets, item_setup=item_setup, setups=_hip_setups())


def _parent(h, case):
    """mpe_solve_bruteforce_batch per set-up, scattered into item order."""
    n = len(case["dets"])
    rec = np.zeros(n, mpe.RESULT_DTYPE)
    hist = np.zeros((n, mpe.binding.MAX_DETECTIONS, mpe.binding.MAX_MARKERS), np.uint32)
    corr = np.zeros((n, mpe.binding.MAX_MARKERS, 2), np.uint32)
    for s, (M, K, D, P) in enumerate(case["setups"]):
        idx = [i for i, t in enumerate(case["item_setup"]) if t == s]
        if not idx:
            continue
        r, hh, c = h.solve_bruteforce_batch([case["dets"][i] for i in idx], M, K, P)
        rec[idx], hist[idx], corr[idx] = r, hh, c
    return rec, hist, corr


def _trace_vote_difference(h, det, M, K, tol, arith):
    """The first hypothesis at which the handle's voting arithmetic `arith` and the strict kernel of the same powers
    (4 for 3, 0 for 1) cast different votes, narrowed down with mpe_vote_items -> text for the assertion."""
    strict = 4 if arith in (3, 4) else 0
    nd, nm = len(det), len(M)
    lo, hi = 0, nd * (nd - 1) * (nd - 2) // 6 * nm * (nm - 1) * (nm - 2)
    while hi - lo > 1:
        edges = np.unique(np.linspace(lo, hi, 65).astype(np.int64))
        a, b = edges[:-1].astype(np.int32), edges[1:].astype(np.int32)
        h.set_option("vote_arith", arith)
        va = h.vote_items(det, M, K, tol, a, b)
        h.set_option("vote_arith", strict)
        vs = h.vote_items(det, M, K, tol, a, b)
        h.set_option("vote_arith", arith)
        bad = [k for k in range(len(a)) if not np.array_equal(va[k], vs[k])]
        if not bad:
            return "no single hypothesis range of [%d, %d) votes differently under vote_arith %d and %d" % (lo, hi, arith, strict)
        lo, hi = int(a[bad[0]]), int(b[bad[0]])
    return "hypothesis %d votes differently under vote_arith %d and %d" % (lo, arith, strict)


def _assert_same(h, case, got, ref, arith):
    for i in range(len(case["dets"])):
        same = [got[k][i].tobytes() == ref[k][i].tobytes() for k in range(3)]
        if all(same):
            continue
        M, K, D, P = case["setups"][case["item_setup"][i]]
        why = ""
        if not same[1] and len(case["dets"][i]) >= 4:
            why = _trace_vote_difference(h, case["dets"][i], M, K, P.back_projection_pixel_tolerance, arith)
        assert False, ("item %d (set-up %d, %d detections): record / histogram / correspondences equal: %s; %s"
                       % (i, case["item_setup"][i], len(case["dets"][i]), same, why))


@pytest.mark.gpu
@pytest.mark.parametrize("arith", [3, 1, 4, 2])
def test_equals_parent_entry_per_setup(handle, case, arith):
    """14 items over three set-ups (a fourth is named by none): out, hist and corr equal those of
    mpe_solve_bruteforce_batch per set-up byte for byte — with the default voting arithmetic, with 1 and 4, and with 2
    through the delegation (one submission per set-up that has items)."""
    h = handle
    h.set_option("vote_arith", arith)
    try:
        c0 = h.get_option("bruteforce_submits")
        got = h.solve_bruteforce_batch_setups(case["dets"], case["setups"], case["item_setup"])
        assert h.get_option("bruteforce_submits") - c0 == (3 if arith == 2 else 1)
        ref = _parent(h, case)
        _assert_same(h, case, got, ref, arith)
    finally:
        h.set_option("vote_arith", 3)


@pytest.mark.gpu
def test_items_match_the_oracle(handle, case, orc):
    """The same items against the CPU oracle's solve_bruteforce, as tests/test_gpu_parity.py holds mpe_solve_bruteforce
    against it: histograms integer-equal, correspondences equal, poses within POS_TOL_M / ROT_TOL_RAD."""
    rec, hist, corr = handle.solve_bruteforce_batch_setups(case["dets"], case["setups"], case["item_setup"])
    specs = _setup_specs()
    posed = {0: 0, 1: 0, 2: 0}
    unposed = 0
    for i, det in enumerate(case["dets"]):
        s = case["item_setup"][i]
        M, K, D, kw = specs[s]
        ro = orc.solve_bruteforce(det, M, K, orc.make_params(**kw))
        nd, nm = len(det), len(M)
        assert np.array_equal(hist[i, :nd, :nm], ro["hist"][:nd]), i
        assert not hist[i, nd:].any() and not hist[i, :, nm:].any(), i
        assert rec["status"][i] == ro["status"], (i, rec["status"][i], ro["status"])
        assert rec["n_det"][i] == nd and rec["n_corr"][i] == ro["n_corr"], i
        assert np.array_equal(corr[i, :ro["n_corr"]], ro["corr"]), i
        if ro["status"] == 0:
            posed[s] += 1
            dp, dr = pose_diff(rec["T"][i].reshape(4, 4), ro["T"])
            assert dp <= POS_TOL_M and dr <= ROT_TOL_RAD, (i, dp, dr)
            assert np.allclose(rec["cov"][i].reshape(6, 6), ro["cov"], rtol=1e-6, atol=1e-12), i
        else:
            unposed += 1
    assert all(v >= 1 for v in posed.values()), posed
    assert unposed >= 1


@pytest.mark.gpu
def test_item_order_permutes_the_records_and_nothing_else(handle, case):
    rec, hist, corr = handle.solve_bruteforce_batch_setups(case["dets"], case["setups"], case["item_setup"])
    perm = np.random.default_rng(77).permutation(len(case["dets"]))
    r2, h2, c2 = handle.solve_bruteforce_batch_setups([case["dets"][i] for i in perm], case["setups"],
                                                      [case["item_setup"][i] for i in perm])
    assert r2.tobytes() == rec[perm].tobytes()
    assert h2.tobytes() == hist[perm].tobytes() and c2.tobytes() == corr[perm].tobytes()


@pytest.mark.gpu
def test_degenerate_calls(handle, case):
    """n = 1 equals mpe_solve_bruteforce; one set-up with item_setup NULL equals the uniform entry; one submission each."""
    h = handle
    i = 1
    s = case["item_setup"][i]
    M, K, D, P = case["setups"][s]
    det = case["dets"][i]
    c0 = h.get_option("bruteforce_submits")
    rec, hist, corr = h.solve_bruteforce_batch_setups([det], case["setups"], [s])
    assert h.get_option("bruteforce_submits") - c0 == 1
    one = h.solve_bruteforce(det, M, K, P)
    assert rec["status"][0] == one["status"] == 0
    assert rec["T"][0].tobytes() == one["T"].tobytes() and rec["cov"][0].tobytes() == one["cov"].tobytes()
    assert (rec["n_det"][0], rec["n_corr"][0], rec["gn_iterations"][0]) == (one["n_det"], one["n_corr"], one["gn_iterations"])
    assert np.array_equal(hist[0, :len(det), :len(M)], one["hist"]) and np.array_equal(corr[0, :one["n_corr"]], one["corr"])
    idx = [k for k, t in enumerate(case["item_setup"]) if t == s]
    dets = [case["dets"][k] for k in idx]
    c0 = h.get_option("bruteforce_submits")
    got = h.solve_bruteforce_batch_setups(dets, [case["setups"][s]], None)
    assert h.get_option("bruteforce_submits") - c0 == 1
    ref = h.solve_bruteforce_batch(dets, M, K, P)
    for k in range(3):
        assert got[k].tobytes() == ref[k].tobytes(), k


@pytest.mark.gpu
def test_mixed_call_is_one_submission(handle, case):
    c0 = handle.get_option("bruteforce_submits")
    handle.solve_bruteforce_batch_setups(case["dets"], case["setups"], case["item_setup"])
    assert handle.get_option("bruteforce_submits") - c0 == 1


N_SEQ = 12
BLANK = 6   # streams 1 and 2 (set-ups 1 and 2) see a black frame here; from the next frame on the object is somewhere
            # else (another trajectory): the predicted pixels match nothing and both streams initialise again, together


def _sequences():
    cams = [None, _camera_b(), _camera_c()]
    cfgs = ["C1", "C2", "C3"]
    kws = [{}, {}, dict(back_projection_pixel_tolerance=2.0)]
    seqs = []
    for j in range(9):
        q = synth.make_sequence(cfgs[j % 3], N_SEQ, seed=1300 + j, camera=cams[j % 3])
        if j in (1, 2):
            q["frames"][BLANK] = 0
            q["frames"][BLANK + 1:] = synth.make_sequence(cfgs[j % 3], N_SEQ, seed=1400 + j, camera=cams[j % 3])["frames"][BLANK + 1:]
        seqs.append(q)
    return seqs, [kws[j % 3] for j in range(9)]


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["mixed", "device"])
def test_driver_initialises_all_setups_in_one_submission(entry):
    """Nine cold trackers on one handle, three per set-up: the first time step initialises every stream by brute force
    in ONE submission, the step after the black frame re-initialises two streams of different set-ups in one again, and
    records and info over the whole sequence are those of Tracker.estimate per stream."""
    seqs, kws = _sequences()
    h, h1 = mpe.Handle(0), mpe.Handle(0)
    ts = [mpe.Tracker(h, q["markers"], q["K"], q["D"], mpe.demo_params(**kw)) for q, kw in zip(seqs, kws)]
    t1 = [mpe.Tracker(h1, q["markers"], q["K"], q["D"], mpe.demo_params(**kw)) for q, kw in zip(seqs, kws)]
    try:
        if entry == "device":
            import torch
            dev = [torch.from_numpy(q["frames"]).cuda() for q in seqs]
        for k in range(N_SEQ):
            times = [seqs[0]["times"][k]] * len(seqs)
            c0 = h.get_option("bruteforce_submits")
            if entry == "device":
                rec, info, upd = mpe.tracker_estimate_batch_device(ts, [d[k] for d in dev], times)
            else:
                rec, info, upd = mpe.tracker_estimate_batch_mixed(ts, [q["frames"][k] for q in seqs], times)
            grew = h.get_option("bruteforce_submits") - c0
            if k == 0:
                assert (info[:, 7] == 1).all(), info[:, 7]
                assert grew == 1
            if k == BLANK + 1:
                assert info[1, 7] == 1 and info[2, 7] == 1, info[:, 7]
                assert grew == 1
            if not info[:, 7].any():
                assert grew == 0, k
            for j, q in enumerate(seqs):
                r = t1[j].estimate(q["frames"][k], q["times"][k])
                assert r["updated"] == bool(upd[j]) == (rec["status"][j] == 0), (k, j)
                assert rec["T"][j].tobytes() == r["T"].tobytes() and rec["cov"][j].tobytes() == r["cov"].tobytes(), (k, j)
                assert tuple(info[j, 0:4]) == r["roi"] and info[j, 4] == r["it_since_initialized"], (k, j)
                assert info[j, 5] == r["n_det"] and info[j, 6] == r["n_corr"], (k, j)
                assert bool(info[j, 7]) == r["used_bruteforce"], (k, j)
        assert (rec["status"] == 0).sum() >= 6   # (the streams track at the end of the sequence)
    finally:
        for t in ts + t1:
            t.close()
        h.close()
        h1.close()
