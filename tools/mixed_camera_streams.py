"""Lock-step tracking of N camera streams, three ways, in one process (8 and 64 streams, ~200 time steps each):

  A  one shared set-up (camera, markers, parameters), one handle: mpe_tracker_run_sequences_batch;
  B  a distinct set-up per stream (every camera its own K and D), one handle: mpe_tracker_run_sequences_batch_mixed_threads;
  C  the same distinct set-ups the way it had to be done before B existed: one handle per set-up,
     mpe_tracker_run_sequences_batch_threads on 4 host threads.

One JSON line per (streams, way): milliseconds per time step and tracked frames per second, then one summary line per
stream count with B / A and C / B.  B's records must equal C's byte for byte (asserted).

The frames: 8 rendered trajectories (README camera, 5 LEDs) played forwards and backwards; stream j shows trajectory
j % 8.  Stream j's set-up in B / C is that camera with fx, fy, cx, cy and k1 moved by a few parts in 10^4 * j: distinct
set-ups, the same work per frame as A.

    python tools/mixed_camera_streams.py [--streams 8,64] [--steps 200] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rpg_monocular_pose_estimator_amd as mpe  # noqa: E402
from rpg_monocular_pose_estimator_amd import synth  # noqa: E402

BASE = 50       # frames of a rendered trajectory
N_TRAJ = 8      # rendered trajectories
WARMUP = 12     # time steps of the untimed run in front of every timed one


def ping_pong(n_steps):
    idx, k, d = [], 0, 1
    for _ in range(n_steps):
        idx.append(k)
        if not 0 <= k + d < BASE:
            d = -d
        k += d
    return np.array(idx)


def camera_of(j, K, D):
    K = K.copy()
    D = D.copy()
    K[0, 0] *= 1.0 + 3e-4 * j
    K[1, 1] *= 1.0 + 2e-4 * j
    K[0, 2] += 0.01 * j
    K[1, 2] -= 0.01 * j
    D[0] *= 1.0 + 1e-4 * j
    return K, D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="8,64")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--threads", type=int, default=4, help="host threads of way C")
    ap.add_argument("--ways", default="ABC", help="a subset of ABC (e.g. B alone under a profiler)")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    steps = args.steps
    traj = [synth.make_sequence("C2", BASE, seed=4200 + s, lin_speed=0.08, ang_speed=0.3) for s in range(N_TRAJ)]
    idx = ping_pong(steps)
    frames = [np.ascontiguousarray(q["frames"][idx]) for q in traj]
    times = np.arange(steps) * 0.02
    M, K0, D0 = traj[0]["markers"], traj[0]["K"], traj[0]["D"]
    P = mpe.demo_params()
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    def timed(make, run, fr):
        """warm-up run on fresh trackers, then the timed run on fresh trackers -> (seconds, records, info)"""
        ts, hs = make()
        run(ts, [f[:WARMUP] for f in fr], times[:WARMUP])
        for t in ts:
            t.close()
        ts2, _ = make(hs)
        t0 = time.perf_counter()
        rec, info = run(ts2, fr, times)
        dt = time.perf_counter() - t0
        for t in ts2:
            t.close()
        for h in hs:
            h.close()
        return dt, rec, info

    for n in [int(x) for x in args.streams.split(",")]:
        fr = [frames[j % N_TRAJ] for j in range(n)]
        cams = [camera_of(j, K0, D0) for j in range(n)]

        def make_a(hs=None):
            hs = hs or [mpe.Handle(0)]
            return [mpe.Tracker(hs[0], M, K0, D0, P) for _ in range(n)], hs

        def make_b(hs=None):
            hs = hs or [mpe.Handle(0)]
            return [mpe.Tracker(hs[0], M, cams[j][0], cams[j][1], P) for j in range(n)], hs

        def make_c(hs=None):
            hs = hs or [mpe.Handle(0) for _ in range(n)]
            return [mpe.Tracker(hs[j], M, cams[j][0], cams[j][1], P) for j in range(n)], hs

        ways = {
            "A": (make_a, lambda ts, f, t: mpe.tracker_run_sequences_batch(ts, f, t)),
            "B": (make_b, lambda ts, f, t: mpe.tracker_run_sequences_batch_mixed(ts, f, t)),
            "C": (make_c, lambda ts, f, t: mpe.tracker_run_sequences_batch(ts, f, t, threads=args.threads)),
        }
        got = {}
        for w, (make, run) in ways.items():
            if w not in args.ways:
                continue
            dt, rec, info = timed(make, run, fr)
            got[w] = (dt, rec, info)
            ms = dt * 1e3 / steps
            emit(dict(tool="mixed_camera_streams", way=w, streams=n, steps=steps, ms_per_step=round(ms, 4),
                      tracked_frames_per_s=round(n * steps / dt, 1),
                      poses=int((rec["status"] == 0).sum()), brute_force_frames=int(info[:, :, 7].sum())))
        if len(got) < 3:
            continue
        assert got["B"][1].tobytes() == got["C"][1].tobytes(), "B and C records differ"
        assert np.array_equal(got["B"][2], got["C"][2]), "B and C step information differs"
        a, b, c = (got[w][0] for w in "ABC")
        emit(dict(tool="mixed_camera_streams", summary=True, streams=n, steps=steps, b_over_a=round(b / a, 3),
                  c_over_b=round(c / b, 3), b_records_equal_c=True))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
