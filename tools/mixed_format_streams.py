"""Lock-step tracking of a rig whose cameras differ in image format: 64 tracked C2 streams on device frames, 32 mono8 and
32 bgr8, 64 time steps from cold trackers, in one process:

  a  ONE lock-step group of 64 on one handle through mpe_tracker_run_sequences_batch_formats_threads — one submission
     per time step, the ROI gather decodes every slot by its own format (k_gather_rois_formats);
  b  what the entries with one format per call need: two groups of 32 on two handles, each through
     mpe_tracker_run_sequences_batch_device_encoded_threads.  One call holds one encoding, so the two groups are two
     calls, made from two host threads at once (b) and one after the other (b_seq);
  c  a single-format group of 64 bgr8 streams through the new entry (c_new) and through the old one (c_old): the new
     entry hands such a group to the old submission, the figures must agree.

Three alternating repetitions, each a warm-up run and a timed run on fresh trackers and handles.  One JSON line per (way,
repetition): tracked frames per second, submissions per time step (option "track_batch_submits") and the host-side split
of the submissions (option "track_profile": pack / enqueue / wait, microseconds per submission); then a summary line
that says whether a is slower than b by more than the spread of b's repetitions.  The records of every way must equal
those of way a stream by stream (asserted).  The lines are appended to profiles/mixed_format_streams.jsonl.

The frames: 8 rendered trajectories (README camera, 5 LEDs); stream j shows trajectory j % 8, the streams 0 .. 31 as
mono8 and 32 .. 63 as bgr8 (B = the rendered frame, G and R = it plus noise in [-6, 6]).

    python tools/mixed_format_streams.py [--streams 64] [--steps 64] [--reps 3] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rpg_monocular_pose_estimator_amd as mpe  # noqa: E402
from rpg_monocular_pose_estimator_amd import synth  # noqa: E402

N_TRAJ = 8      # rendered trajectories
WARMUP = 12     # time steps of the untimed run in front of every timed one


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_format_streams.jsonl"))
    args = ap.parse_args()
    n, steps, half = args.streams, args.steps, args.streams // 2
    lib = mpe.load_library()
    traj = [synth.make_sequence("C2", steps, seed=4200 + s, lin_speed=0.08, ang_speed=0.3) for s in range(N_TRAJ)]
    rows, cols = int(traj[0]["rows"]), int(traj[0]["cols"])
    mono = torch.from_numpy(np.stack([q["frames"] for q in traj])).cuda()           # (N_TRAJ, steps, rows, cols)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    v = mono.to(torch.int32)
    noisy = lambda: (v + torch.randint(-6, 7, v.shape, device="cuda", generator=gen, dtype=torch.int32)).clamp_(0, 255).to(torch.uint8)
    bgr = torch.stack([mono, noisy(), noisy()], -1)                                 # (N_TRAJ, steps, rows, cols, 3)
    del v
    torch.cuda.synchronize()
    times = np.arange(steps) * 0.02
    M, K0, D0, P = traj[0]["markers"], traj[0]["K"], traj[0]["D"], mpe.demo_params()
    dp = C.POINTER(C.c_double)
    tp = times.ctypes.data_as(dp)
    ENC_BGR8 = mpe.ENCODINGS["bgr8"]
    F_MONO = mpe.ImageFormat(rows, cols, cols, mpe.ENCODINGS["mono8"], 0)
    F_BGR = mpe.ImageFormat(rows, cols, 3 * cols, ENC_BGR8, 0)
    mono_ptr = lambda j: mono[j % N_TRAJ].data_ptr()
    bgr_ptr = lambda j: bgr[j % N_TRAJ].data_ptr()
    # stream j < half: mono8, else bgr8
    mixed_ptrs = (C.c_void_p * n)(*([mono_ptr(j) for j in range(half)] + [bgr_ptr(j) for j in range(half, n)]))
    mixed_fmts = (mpe.ImageFormat * n)(*([F_MONO] * half + [F_BGR] * (n - half)))
    mixed_fstr = (C.c_size_t * n)(*([rows * cols] * half + [rows * cols * 3] * (n - half)))
    all_bgr_ptrs = (C.c_void_p * n)(*[bgr_ptr(j) for j in range(n)])
    all_bgr_fmts = (mpe.ImageFormat * n)(*([F_BGR] * n))
    all_bgr_fstr = (C.c_size_t * n)(*([rows * cols * 3] * n))
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    def formats_call(ts, ptrs, fmts, fstr, n_steps, rec, info):
        m = len(ts)
        rc = lib.mpe_tracker_run_sequences_batch_formats_threads((C.c_void_p * m)(*[t._t for t in ts]), m, ptrs, n_steps, 1, fmts,
                                                                 fstr, tp, rec.ctypes.data, info.ctypes.data, 1)
        assert rc >= 0, (rc, lib.mpe_last_error(ts[0]._handle._h).decode())

    def encoded_call(ts, ptrs, enc, bpp, n_steps, rec, info):
        m = len(ts)
        rc = lib.mpe_tracker_run_sequences_batch_device_encoded_threads((C.c_void_p * m)(*[t._t for t in ts]), m, ptrs, n_steps,
                                                                        rows, cols, cols * bpp, rows * cols * bpp, enc, 0, tp,
                                                                        rec.ctypes.data, info.ctypes.data, 1)
        assert rc >= 0, (rc, lib.mpe_last_error(ts[0]._handle._h).decode())

    def run(way, hs, n_steps):
        """fresh trackers on the handles hs, n_steps time steps -> (records, info, seconds)"""
        rec, info = np.zeros((n, n_steps), mpe.RESULT_DTYPE), np.zeros((n, n_steps, 8), np.int32)
        mk = lambda h, m: [mpe.Tracker(h, M, K0, D0, P) for _ in range(m)]
        if way == "a":
            ts = mk(hs[0], n)
            jobs = [lambda: formats_call(ts, mixed_ptrs, mixed_fmts, mixed_fstr, n_steps, rec, info)]
        elif way in ("b", "b_seq"):
            ts = mk(hs[0], half) + mk(hs[1], n - half)
            lo = (C.c_void_p * half)(*mixed_ptrs[:half])
            hi = (C.c_void_p * (n - half))(*mixed_ptrs[half:])
            jobs = [lambda: encoded_call(ts[:half], lo, 0, 1, n_steps, rec[:half], info[:half]),
                    lambda: encoded_call(ts[half:], hi, ENC_BGR8, 3, n_steps, rec[half:], info[half:])]
        elif way == "c_new":
            ts = mk(hs[0], n)
            jobs = [lambda: formats_call(ts, all_bgr_ptrs, all_bgr_fmts, all_bgr_fstr, n_steps, rec, info)]
        else:
            ts = mk(hs[0], n)
            jobs = [lambda: encoded_call(ts, all_bgr_ptrs, ENC_BGR8, 3, n_steps, rec, info)]
        t0 = time.perf_counter()
        if way == "b":      # (ctypes releases the interpreter lock for the duration of a call)
            th = [threading.Thread(target=j) for j in jobs]
            for t in th:
                t.start()
            for t in th:
                t.join()
        else:
            for j in jobs:
                j()
        dt = time.perf_counter() - t0
        for t in ts:
            t.close()
        return rec, info, dt

    ways = ("a", "b", "b_seq", "c_new", "c_old")
    fps = {w: [] for w in ways}
    us_all = {w: [] for w in ways}
    ref = {}
    for rep in range(args.reps):
        for way in ways:
            hs = [mpe.Handle(0) for _ in range(2 if way in ("b", "b_seq") else 1)]
            run(way, hs, WARMUP)
            for h in hs:
                h.set_option("track_profile", 1)
            c0 = [h.get_option("track_batch_submits") for h in hs]
            rec, info, dt = run(way, hs, steps)
            subs = [h.get_option("track_batch_submits") - c for h, c in zip(hs, c0)]
            us = [{w: round(h.get_option("track_ns_" + w) / 1e3, 2) for w in ("pack", "enqueue", "wait")} for h in hs]
            for h in hs:
                h.close()
            key = "c" if way.startswith("c") else "ab"
            if key not in ref:
                ref[key] = (rec.tobytes(), info.tobytes())
            assert (rec.tobytes(), info.tobytes()) == ref[key], "records of way %s differ (repetition %d)" % (way, rep)
            fps[way].append(n * steps / dt)
            us_all[way].append(us)
            emit(dict(tool="mixed_format_streams", way=way, streams=n, steps=steps, rep=rep, handles=len(hs),
                      ms_per_step=round(dt * 1e3 / steps, 4), tracked_frames_per_s=round(n * steps / dt, 1),
                      submissions_per_step=round(sum(subs) / steps, 3), us_per_submission=us,
                      poses=int((rec["status"] == 0).sum()), brute_force_frames=int(info[:, :, 7].sum())))
    med = {w: float(np.median(fps[w])) for w in ways}
    b = np.array(fps["b"])
    emit(dict(tool="mixed_format_streams", summary=True, streams=n, steps=steps, reps=args.reps,
              tracked_frames_per_s={w: [round(x, 1) for x in fps[w]] for w in ways},
              median_tracked_frames_per_s={w: round(med[w], 1) for w in ways},
              b_spread_frames_per_s=round(float(b.max() - b.min()), 1),
              a_over_b=round(med["a"] / med["b"], 3), a_over_b_seq=round(med["a"] / med["b_seq"], 3),
              a_slower_than_b_by_more_than_b_spread=bool(med["b"] - med["a"] > b.max() - b.min()),
              c_new_over_c_old=round(med["c_new"] / med["c_old"], 3), records_equal=True))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
