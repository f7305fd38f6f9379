"""What the rig's partial-view tracking step costs, for the record (recorded, not gated): the device time of the ONE
launch of mpe_rig_track_batch (option "rig_launch_profile": a pair of events around it, the copies outside) for 1 and
1024 problems of (3 cameras x 5 markers) and (16 x 16) with max_rounds 1 and 2, and beside each the launch of
mpe_rig_optimise_pose_batch over the rows the one-round call matched, from the same starts — the refinement alone.
Every camera sees every marker (0.1 px noise) among 2, 0 and 40 stray detections (the lists the matching phase walks); the
start is 0.004 rad / 0.004 m off.  The median of 7 calls behind a warm-up call.  All configurations run in ONE child process under one time limit; a failure ends the
tool.
    python tools/rig_tracking_numbers.py [profiles/rig_tracking.jsonl]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = [(3, 5), (16, 16)]      # cameras, markers
BATCHES = (1, 1024)
STRAY = (2, 0, 40)              # stray detections per camera beside the LEDs: what the matching phase costs per detection
LIMIT = 300                       # seconds for the whole run


def measure():
    import numpy as np
    import rpg_monocular_pose_estimator_amd as mpe
    import witness_rig
    import witness_rig_track as W
    h = mpe.Handle()
    h.set_option("rig_launch_profile", 1)

    def timed(call):
        call()
        ns = []
        for _ in range(7):
            call()
            ns.append(h.get_option("rig_launch_ns"))
        return round(float(np.median(ns)) / 1e3, 2)
    for n_cam, n_mk in CONFIGS:
        for stray in STRAY:
            rng = np.random.default_rng(n_cam)
            cameras = witness_rig.random_cameras(rng, n_cam)
            markers = rng.uniform(-0.5 if n_mk > 8 else -0.25, 0.5 if n_mk > 8 else 0.25, (n_mk, 3))
            items = [W.random_problem(rng, rig=(cameras, markers), seen=[n_mk] * n_cam, clutter=stray)[0]
                     for _ in range(max(BATCHES))]
            tol_m, tol_a = items[0][4], items[0][5]
            for n in BATCHES:
                dets, T0 = [it[2] for it in items[:n]], [it[3] for it in items[:n]]
                rec, match, info = h.rig_track_batch(cameras, markers, dets, T0, tol_m, tol_a, max_rounds=1)
                rows = [W.rows_of(match[i].astype(np.int64), markers, dets[i]) for i in range(n)]
                rec2, _, info2 = h.rig_track_batch(cameras, markers, dets, T0, tol_m, tol_a, max_rounds=2)
                print(json.dumps(dict(
                    cameras=n_cam, markers=n_mk, detections_per_camera=n_mk + stray, problems=n,
                    rows_mean=round(float(info["rows"].mean()), 1),
                    poses_one_round=int((rec["status"] == 0).sum()), poses_two_rounds=int((rec2["status"] == 0).sum()),
                    gn_iterations_mean=round(float(rec["gn_iterations"].mean()), 2),
                    refinements_two_rounds_mean=round(float(info2["rounds"].mean()), 2),
                    track_us_one_round=timed(lambda: h.rig_track_batch(cameras, markers, dets, T0, tol_m, tol_a, max_rounds=1)),
                    track_us_two_rounds=timed(lambda: h.rig_track_batch(cameras, markers, dets, T0, tol_m, tol_a, max_rounds=2)),
                    refine_us=timed(lambda: h.rig_optimise_pose_batch(cameras, rows, T0)))), flush=True)
    h.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--measure":
        measure()
        sys.exit(0)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure"], capture_output=True, text=True, timeout=LIMIT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit("the measurement failed with %d" % r.returncode)
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    out.write(r.stdout)
