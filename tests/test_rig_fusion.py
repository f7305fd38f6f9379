"""The cameras of a rig fused into one body pose on the device (mpe_rig_optimise_pose_batch / k_rig_refine,
mpe_rig_fuse_trackers, mpe_rig_seed_trackers, Rig): one camera with the identity extrinsic is mpe_optimise_pose bit for
bit; the row-count shapes (fewer than a wave, 65 = one more than a wave, 256 = the cap) against the numpy witness
(tests/witness_rig.py) with the criteria of tests/test_gpu_parity.py:801-804; a record does not depend on the batch it is
in; the refusals; the lock-step group of a 3-camera rig; re-acquisition of a camera that lost the body."""
import ctypes as C

import numpy as np
import pytest

import rpg_monocular_pose_estimator_amd as mpe
from rpg_monocular_pose_estimator_amd import synth
import witness_rig

pytestmark = pytest.mark.gpu


def _same_records(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_one_camera_identity_extrinsic_is_optimise_pose(hip):
    """4 and 5 rows of C2 frames, from the check pose and from two perturbed starts: T, cov and gn_iterations of the rig
    entry (all problems in one call) are those of mpe_optimise_pose, bit for bit."""
    d = synth.make_frames("C2", 6, seed=123)
    Ph = mpe.demo_params()
    cameras = [(d["K"], np.eye(4))]
    problems, starts, want = [], [], []
    for i in range(6):
        und, _ = hip.find_leds(d["frames"][i], Ph, d["K"], d["D"])
        r = hip.solve_bruteforce(und, d["markers"], d["K"], Ph)
        if r["status"] != 0 or r["n_corr"] != 5:
            continue                                     # (a frame the brute force leaves without a pose brings no rows)
        ok, T0 = hip.check_correspondences(und, d["markers"], d["K"], Ph, r["corr"])
        assert ok, i
        rng = np.random.default_rng(i)
        for n_rows in (4, 5):
            corr = r["corr"][:n_rows]
            for trial in range(3):
                Ts = T0.copy()
                if trial:
                    Ts[:3, :3] = synth.rodrigues(rng.normal(size=3), 0.05 * trial) @ Ts[:3, :3]
                    Ts[:3, 3] += rng.normal(0, 0.01 * trial, 3)
                want.append(hip.optimise_pose(und, d["markers"], d["K"], Ph, corr, Ts))
                problems.append([(0, d["markers"][m - 1], und[j - 1]) for m, j in corr])
                starts.append(Ts)
    assert len(want) >= 3 * 6
    rec = hip.rig_optimise_pose_batch(cameras, problems, starts)
    for k, w in enumerate(want):
        assert w["status"] == 0 and rec["status"][k] == 0, k
        assert rec["gn_iterations"][k] == w["gn_iterations"], (k, rec["gn_iterations"][k], w["gn_iterations"])
        assert rec["T"][k].tobytes() == np.ascontiguousarray(w["T"]).tobytes(), k
        assert rec["cov"][k].tobytes() == np.ascontiguousarray(w["cov"]).tobytes(), k
        assert rec["n_corr"][k] == len(problems[k]) and rec["n_det"][k] == 1


@pytest.mark.parametrize("seen,n_markers", [((4, 1), 5), ((5, 3, 2), 5), ((13,) * 5, 13), ((16,) * 16, 16)],
                         ids=["4+1", "5+3+2", "5x13=65", "16x16=256"])
def test_row_count_shapes_against_the_witness(hip, seen, n_markers):
    rng = np.random.default_rng(100 + len(seen))
    cameras, rows, T0 = witness_rig.random_rig(rng, n_cam=len(seen), seen=list(seen), n_markers=n_markers)
    assert len(rows) == sum(seen)
    rec = hip.rig_optimise_pose_batch(cameras, [rows], [T0])[0]
    assert rec["status"] == 0 and rec["n_corr"] == len(rows) and rec["n_det"] == len(seen)
    it = witness_rig.check_against_witness(rec, cameras, rows, T0, seen)
    assert 3 <= it <= 25, it


def test_a_record_does_not_depend_on_its_batch(hip):
    """Calls of 1, 4, 5 and 67 problems of mixed row counts — a 0-row and a 2-row problem between full ones (status 1,
    the neighbours untouched), a 65-row and a 256-row one among them: every record equals the same problem submitted
    alone, bit for bit."""
    rng = np.random.default_rng(31)
    markers = rng.uniform(-0.25, 0.25, (16, 3))
    cameras = witness_rig.random_cameras(rng, 16)
    problems, starts = [], []
    for k in range(67):
        if k == 1:
            seen = [0] * 16                              # no row at all
        elif k == 3:
            seen = [1, 1] + [0] * 14                     # two rows: no pose
        elif k == 2:
            seen = [13] * 5 + [0] * 11                   # 65 rows
        elif k == 4:
            seen = [16] * 16                             # 256 rows
        else:
            seen = [int(rng.integers(4, 17))] + [int(rng.integers(0, 17)) if rng.random() < 0.4 else 0 for _ in range(15)]
        rows, T0 = witness_rig.random_problem(rng, cameras, seen, markers)
        problems.append(rows)
        starts.append(T0)
    alone = np.concatenate([hip.rig_optimise_pose_batch(cameras, [p], [t]) for p, t in zip(problems, starts)])
    assert list(alone["status"][:5]) == [0, 1, 0, 1, 0] and (alone["status"][5:] == 0).all()
    assert list(alone["n_corr"][:5]) == [len(p) for p in problems[:5]] and alone["n_corr"][4] == 256
    for k in (1, 3):
        assert alone["gn_iterations"][k] == 0 and not alone["cov"][k].any()
        assert np.array_equal(alone["T"][k].reshape(4, 4), starts[k])
    witness_rig.check_against_witness(alone[4], cameras, problems[4], starts[4], "256 rows")
    for n in (1, 4, 5, 67):
        rec = hip.rig_optimise_pose_batch(cameras, problems[:n], starts[:n])
        for k in range(n):
            assert _same_records(rec[k], alone[k]), (n, k)
    # ... and on where the batch begins: the rows of a call need not start at row 0 of the caller's arrays
    rec = hip.rig_optimise_pose_batch(cameras, problems[60:], starts[60:])
    assert _same_records(rec, alone[60:])


def _raw_batch(hip, n_cameras, begin, cam, n_problems, T_init=True, sentinel=0x5a):
    lib = hip._lib
    cams = (mpe.MpeRigCamera * 17)()
    for c in cams:
        c.K[:] = [400, 0, 370, 0, 400, 240, 0, 0, 1]
        c.T_cam_rig[:] = np.eye(4).reshape(16)
    begin = np.ascontiguousarray(begin, np.int32)
    cam = np.ascontiguousarray(cam, np.int32)
    n_rows = max(len(cam), 1)
    xyz = np.tile([0.1, 0.05, 0.0], (n_rows, 1)) * np.arange(1, n_rows + 1)[:, None] / n_rows
    uv = np.tile([380.0, 250.0], (n_rows, 1))
    T0 = np.tile(np.eye(4).reshape(16), (max(n_problems, 1), 1))
    T0[:, 11] = 1.5
    rec = np.full(max(n_problems, 1) * mpe.RESULT_DTYPE.itemsize, sentinel, np.uint8)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    rc = lib.mpe_rig_optimise_pose_batch(hip._h, cams, n_cameras, begin.ctypes.data_as(ip), cam.ctypes.data_as(ip),
                                         xyz.ctypes.data_as(dp), uv.ctypes.data_as(dp), n_problems,
                                         T0.ctypes.data_as(dp) if T_init else None, rec.ctypes.data)
    return rc, lib.mpe_last_error(hip._h).decode(), bool((rec == sentinel).all())


def test_refusals(hip):
    """Every refusal returns its code, mpe_last_error names it, and no record is written."""
    ERR_ARG, ERR_UNSUPPORTED = -1, -3
    ok_cam = [0, 1, 2, 3]
    rc, msg, clean = _raw_batch(hip, 16, [0, 4], [0, 1, 16, 3], 1)
    assert rc == ERR_ARG and "camera index" in msg and clean
    rc, msg, clean = _raw_batch(hip, 16, [0, 257], [k % 16 for k in range(257)], 1)
    assert rc == ERR_UNSUPPORTED and "rows" in msg and clean
    for n_cameras in (0, 17):
        rc, msg, clean = _raw_batch(hip, n_cameras, [0, 4], ok_cam, 1)
        assert rc == ERR_ARG and "n_cameras" in msg and clean, n_cameras
    rc, msg, clean = _raw_batch(hip, 4, [0, 4], ok_cam, 1, T_init=False)
    assert rc == ERR_ARG and "T_init" in msg and clean
    rc, msg, clean = _raw_batch(hip, 4, [0, 4, 2], ok_cam, 2)
    assert rc == ERR_ARG and "row_begin" in msg and clean
    rc, msg, clean = _raw_batch(hip, 4, [0], [], 0)          # nothing to do, nothing submitted
    assert rc == 0 and clean
    rc, msg, clean = _raw_batch(hip, 4, [0, 4], ok_cam, 1)   # (the helper's call as such is a good one)
    assert rc == 0 and not clean
    # mpe_rig_fuse_trackers: one body, one handle
    Ph = mpe.demo_params()
    K, D = synth.camera_for(480, 752)
    other = mpe.Handle()
    try:
        t0 = mpe.Tracker(hip, synth.M5, K, D, Ph)
        t1 = mpe.Tracker(hip, synth.M4, K, D, Ph)
        t2 = mpe.Tracker(other, synth.M5, K, D, Ph)
        E = np.tile(np.eye(4), (2, 1, 1))
        for pair, word in (((t0, t1), "marker set"), ((t0, t2), "one handle"), ((t0, t0), "twice")):
            with pytest.raises(mpe.MpeError, match=word):
                mpe.Rig(hip, pair, E).fuse()
        fused, rec, rows = mpe.Rig(hip, (t0,), E[:1]).fuse()    # a tracker that has seen no frame brings no row
        assert not fused and rec["status"][0] == 1 and rows[0] == 0
        for t in (t0, t1, t2):
            t.close()
    finally:
        other.close()


def _rig_cameras(n):
    """n cameras of C2's image size on a 12 cm base line, turned a few degrees towards each other; camera 0 is the rig
    frame."""
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


def _trackers(hip, seq, cams):
    Ph = mpe.demo_params()
    return [mpe.Tracker(hip, seq["markers"], K, D, Ph) for K, D in cams]


def test_lock_step_rig(hip):
    """A 3-camera rig through Rig.step: the per-camera records are those of the same lock-step call without a rig, byte
    for byte; the rig record is mpe_rig_optimise_pose_batch over the rows read back through the getters, bit for bit,
    and within the criteria of the witness."""
    cams, E = _rig_cameras(3)
    seq = synth.make_rig_sequence("C2", 8, 5, cams, E)
    plain = _trackers(hip, seq, cams)
    rigged = _trackers(hip, seq, cams)
    rig = mpe.Rig(hip, rigged, E)
    n_fused = 0
    for k in range(8):
        imgs = [f[k] for f in seq["frames"]]
        times = [seq["times"][k]] * 3
        want = mpe.tracker_estimate_batch_mixed(plain, imgs, times)
        rec, info, upd, rr, fused = rig.step(imgs, times)
        assert _same_records(rec, want[0]) and np.array_equal(info, want[1]) and np.array_equal(upd, want[2]), k
        assert upd.all() and fused, k                    # (the precondition of what follows: the seed was chosen for it)
        rows = []
        for c, t in enumerate(rigged):
            xy = t.image_points()
            rows += [(c, seq["markers"][m - 1], xy[j - 1]) for m, j in t.correspondences()]
        assert len(rows) == int(rr["n_corr"][0]) == int(info[:, 6].sum()) and rr["n_det"][0] == 3, k
        cameras = [(K, E[c]) for c, (K, _) in enumerate(cams)]
        T0 = rec["T"][0].reshape(4, 4)                   # (E_0 is the identity: the start is camera 0's pose as it is)
        again = hip.rig_optimise_pose_batch(cameras, [rows], [T0])
        assert _same_records(again, rr), k
        witness_rig.check_against_witness(rr[0], cameras, rows, T0, k)
        # the fused pose is the body's: a few tenths of a millimetre from the truth
        assert np.abs(rr["T"][0].reshape(4, 4) - seq["T_true"][k])[:3, 3].max() < 5e-3, k
        n_fused += 1
    assert n_fused == 8
    for t in plain + rigged:
        t.close()


# A tracker that misses two frames is not reset (as the reference's is not): on frame 6 it extrapolates its poses of
# frames 2 and 3 over three steps.  With make_sequence's gentle motion that prediction is within a pixel or two and the
# frame tracks all the same; the body of this sequence moves fast enough (1 m/s, 8 rad/s) that the stale prediction is
# some 8 px off — beyond nearest_neighbour_pixel_tolerance (7) — while every one-step prediction stays within 3 px.
# The seed is one for which the plain run has a pose on every other frame (asserted below).
LOST_BODY = dict(seed=1, lin_speed=1.0, ang_speed=8.0)


def test_a_camera_that_lost_the_body_is_seeded_from_the_rig(hip):
    """2 cameras, 10 frames, camera 1 sees only 2 LEDs on frames 4 and 5.  Plain lock-step run: camera 1 runs the brute
    force on frame 6.  With reseed=True it tracks instead — a ROI smaller than the image, no brute force, the frame
    updates, the same pose to 1e-9 — and camera 0's records are byte-identical in both runs."""
    cams, E = _rig_cameras(2)
    seq = synth.make_rig_sequence("C2", 10, dropout={1: (4, 5)}, cameras=cams, T_cam_rig=E, **LOST_BODY)
    runs = {}
    for reseed in (False, True):
        ts = _trackers(hip, seq, cams)
        rig = mpe.Rig(hip, ts, E)
        out = []
        for k in range(10):
            out.append(rig.step([f[k] for f in seq["frames"]], [seq["times"][k]] * 2, reseed=reseed))
        runs[reseed] = out
        for t in ts:
            t.close()
    plain, seeded = runs[False], runs[True]
    for k in range(10):                                  # the precondition: a pose on every frame but camera 1's 4 and 5
        assert plain[k][2][0] and bool(plain[k][2][1]) == (k not in (4, 5)), k
    assert plain[6][1][1, 7] == 1                        # plain: camera 1 re-initialises by brute force
    rec, info, upd, rr, fused = seeded[6]
    assert info[1, 7] == 0 and upd[1]
    assert 0 < info[1, 2] * info[1, 3] < 752 * 480       # tracked in a ROI
    assert np.abs(rec["T"][1] - plain[6][0]["T"][1]).max() <= 1e-9
    for k in range(10):
        assert _same_records(seeded[k][0][0], plain[k][0][0]) and np.array_equal(seeded[k][1][0], plain[k][1][0]), k
