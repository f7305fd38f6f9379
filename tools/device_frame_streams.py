"""Lock-step tracking of N camera streams with the frames in pinned host memory against the frames in device memory,
in one process (8 and 64 streams, 200 time steps from cold trackers):

  host    mpe_tracker_run_sequences_batch_mixed_threads over sequences in page-locked host memory (every ROI is cloned
          on the host and copied; whole frames while a stream initialises or retries);
  device  mpe_tracker_run_sequences_batch_device_threads over the same sequences uploaded once, outside the timed region
          (a kernel gathers the ROIs from the device images).

Three alternating repetitions (host, device, host, device, ...), each a warm-up run and a timed run on fresh trackers.
One JSON line per (streams, way, repetition): milliseconds per time step and the host-side split of the submissions
(option "track_profile": pack / enqueue / wait, microseconds per submission), then one summary line per stream count.
The device records must equal the host records byte for byte (asserted).  A third pair of lines times the cold start
alone (the first time step: every stream submits its whole frame).

The frames: 8 rendered trajectories (README camera, 5 LEDs) played forwards and backwards; stream j shows trajectory
j % 8.

    python tools/device_frame_streams.py [--streams 8,64] [--steps 200] [--reps 3] [--out FILE]
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
COLD_REPS = 20  # cold first steps timed per way and repetition


def ping_pong(n_steps):
    idx, k, d = [], 0, 1
    for _ in range(n_steps):
        idx.append(k)
        if not 0 <= k + d < BASE:
            d = -d
        k += d
    return np.array(idx)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="8,64")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    steps = args.steps
    traj = [synth.make_sequence("C2", BASE, seed=4200 + s, lin_speed=0.08, ang_speed=0.3) for s in range(N_TRAJ)]
    idx = ping_pong(steps)
    rows, cols = int(traj[0]["rows"]), int(traj[0]["cols"])
    pinned, device = [], []
    for q in traj:
        pf = mpe.PinnedFrames(steps, rows, cols)
        pf.array[:] = q["frames"][idx]
        pinned.append(pf)
        device.append(torch.from_numpy(pf.array).cuda())
    torch.cuda.synchronize()
    times = np.arange(steps) * 0.02
    M, K0, D0 = traj[0]["markers"], traj[0]["K"], traj[0]["D"]
    P = mpe.demo_params()
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    def run(way, ts, n_steps, n):
        if way == "host":
            return mpe.tracker_run_sequences_batch_mixed(ts, [pinned[j % N_TRAJ].array[:n_steps] for j in range(n)],
                                                         times[:n_steps])
        return mpe.tracker_run_sequences_batch_device(ts, [device[j % N_TRAJ][:n_steps] for j in range(n)], times[:n_steps])

    def split(h):
        return ({w: round(h.get_option("track_ns_" + w) / 1e3, 2) for w in ("pack", "enqueue", "wait")},
                h.get_option("track_steps"))

    for n in [int(x) for x in args.streams.split(",")]:
        ms = {"host": [], "device": []}
        cold = {"host": [], "device": []}
        ref = None
        for rep in range(args.reps):
            for way in ("host", "device"):
                h = mpe.Handle(0)
                mk = lambda: [mpe.Tracker(h, M, K0, D0, P) for _ in range(n)]
                ts = mk()
                run(way, ts, WARMUP, n)
                for t in ts:
                    t.close()
                ts = mk()
                h.set_option("track_profile", 1)
                t0 = time.perf_counter()
                rec, info = run(way, ts, steps, n)
                dt = time.perf_counter() - t0
                us, subs = split(h)
                h.set_option("track_profile", 0)
                for t in ts:
                    t.close()
                if ref is None:
                    ref = (rec.tobytes(), info.tobytes())
                assert (rec.tobytes(), info.tobytes()) == ref, "records of %s frames differ (repetition %d)" % (way, rep)
                ms[way].append(dt * 1e3 / steps)
                emit(dict(tool="device_frame_streams", frames=way, streams=n, steps=steps, rep=rep,
                          ms_per_step=round(dt * 1e3 / steps, 4), tracked_frames_per_s=round(n * steps / dt, 1),
                          submissions=subs, us_per_submission=us, poses=int((rec["status"] == 0).sum()),
                          brute_force_frames=int(info[:, :, 7].sum())))
                # the cold start alone: the first time step of fresh trackers, every stream's whole frame submitted
                t_cold = []
                for _ in range(COLD_REPS):
                    ts = mk()
                    t0 = time.perf_counter()
                    run(way, ts, 1, n)
                    t_cold.append((time.perf_counter() - t0) * 1e3)
                    for t in ts:
                        t.close()
                cold[way].append(float(np.median(t_cold)))
                emit(dict(tool="device_frame_streams", frames=way, streams=n, rep=rep, cold_first_step_ms=round(cold[way][-1], 4),
                          cold_steps_timed=COLD_REPS))
                h.close()
        hm, dm = np.array(ms["host"]), np.array(ms["device"])
        emit(dict(tool="device_frame_streams", summary=True, streams=n, steps=steps, reps=args.reps,
                  host_ms_per_step=[round(float(v), 4) for v in hm], device_ms_per_step=[round(float(v), 4) for v in dm],
                  host_spread_ms=round(float(hm.max() - hm.min()), 4),
                  device_over_host=round(float(np.median(dm) / np.median(hm)), 3),
                  cold_first_step_host_ms=round(float(np.median(cold["host"])), 4),
                  cold_first_step_device_ms=round(float(np.median(cold["device"])), 4),
                  device_records_equal_host=True))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for pf in pinned:
        pf.close()


if __name__ == "__main__":
    main()
