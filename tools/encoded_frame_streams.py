"""Lock-step tracking of N camera streams whose frames are in device memory in the camera's own encoding (bgr8 and
mono16; 8 and 64 streams, 200 time steps from cold trackers), two ways in one process:

  A  mpe_convert_to_mono8 of the time step's N frames into a device mono8 buffer (one call, one launch), then
     mpe_tracker_estimate_batch_device over that buffer — what a caller does without the encoded entries;
  B  mpe_tracker_estimate_batch_device_encoded over the encoded frames (the ROI gather decodes what it gathers; no mono8
     copy, no conversion launch).

Both ways are the same Python loop over the time steps around prepared ctypes calls; the N frames of a time step are
one contiguous (N, rows, cols, bytes per pixel) block, generated on the device outside the timed region.  Three
alternating repetitions (A, B, A, B, ...), each a warm-up run and a timed run on fresh trackers.  One JSON line per
(encoding, streams, way, repetition): milliseconds per time step and the host-side split of the submissions (option
"track_profile": pack / enqueue / wait, microseconds per submission), one line for the cold first step (every stream's
whole frame), one for the conversion launch of way A alone, then a summary line per (encoding, streams).  The records
of B must equal those of A byte for byte (asserted).

The frames: 8 rendered trajectories (README camera, 5 LEDs) played forwards and backwards; stream j shows trajectory
j % 8.  bgr8: B = the rendered frame, G and R = it plus noise in [-6, 6]; mono16: the frame * 257 plus noise in
[-128, 128].

    python tools/encoded_frame_streams.py [--streams 8,64] [--encodings bgr8,mono16] [--steps 200] [--reps 3] [--out FILE]
"""
import argparse
import ctypes as C
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
BPP = {"bgr8": 3, "mono16": 2}


def ping_pong(n_steps):
    idx, k, d = [], 0, 1
    for _ in range(n_steps):
        idx.append(k)
        if not 0 <= k + d < BASE:
            d = -d
        k += d
    return np.array(idx)


def encode_on_device(f, encoding, gen):
    """f: (..., rows, cols) uint8 CUDA tensor -> (..., rows, cols, bytes per pixel) uint8."""
    import torch
    v = f.to(torch.int32)
    if encoding == "mono16":
        v = (v * 257 + torch.randint(-128, 129, v.shape, device=f.device, generator=gen, dtype=torch.int32)).clamp_(0, 65535)
        return torch.stack([(v & 255).to(torch.uint8), (v >> 8).to(torch.uint8)], -1)    # little-endian
    noisy = lambda: (v + torch.randint(-6, 7, v.shape, device=f.device, generator=gen, dtype=torch.int32)).clamp_(0, 255).to(torch.uint8)
    return torch.stack([f, noisy(), noisy()], -1)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="8,64")
    ap.add_argument("--encodings", default="bgr8,mono16")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    steps = args.steps
    lib = mpe.load_library()
    traj = [synth.make_sequence("C2", BASE, seed=4200 + s, lin_speed=0.08, ang_speed=0.3) for s in range(N_TRAJ)]
    idx = ping_pong(steps)
    rows, cols = int(traj[0]["rows"]), int(traj[0]["cols"])
    d_traj = torch.from_numpy(np.stack([q["frames"] for q in traj])).cuda()    # (N_TRAJ, BASE, rows, cols)
    times = np.arange(steps) * 0.02
    M, K0, D0 = traj[0]["markers"], traj[0]["K"], traj[0]["D"]
    P = mpe.demo_params()
    lines = []
    dp = C.POINTER(C.c_double)

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    for encoding in args.encodings.split(","):
        bpp, enc = BPP[encoding], mpe.binding.ENCODINGS[encoding]
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7)
        e_traj = encode_on_device(d_traj, encoding, gen)                        # (N_TRAJ, BASE, rows, cols, bpp)
        for n in [int(x) for x in args.streams.split(",")]:
            # the N frames of time step k: one contiguous block
            pick = torch.from_numpy(np.arange(n) % N_TRAJ).cuda()
            frames = torch.stack([e_traj[pick, int(k)] for k in idx])            # (steps, N, rows, cols, bpp)
            mono = torch.empty((n, rows, cols), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            fbytes = rows * cols * bpp
            enc_ptrs = [(C.c_void_p * n)(*[frames[k].data_ptr() + j * fbytes for j in range(n)]) for k in range(steps)]
            mono_ptrs = (C.c_void_p * n)(*[mono.data_ptr() + j * rows * cols for j in range(n)])
            tk = [np.full(n, times[k]) for k in range(steps)]
            rec = np.zeros((steps, n), mpe.RESULT_DTYPE)
            info = np.zeros((steps, n, 8), np.int32)

            def run(way, h, ts, n_steps):
                """the time steps 0 .. n_steps - 1 on trackers ts; the records into rec / info"""
                tsp = (C.c_void_p * n)(*[t._t for t in ts])
                for k in range(n_steps):
                    if way == "A":
                        rc = lib.mpe_convert_to_mono8(h._h, C.c_void_p(frames[k].data_ptr()), 1, enc, 0, n, rows, cols,
                                                      C.c_size_t(cols * bpp), C.c_size_t(fbytes), C.c_void_p(mono.data_ptr()), 1)
                        assert rc == 0, rc
                        rc = lib.mpe_tracker_estimate_batch_device(tsp, n, mono_ptrs, rows, cols, cols, tk[k].ctypes.data_as(dp),
                                                                   rec[k].ctypes.data, info[k].ctypes.data, None)
                    else:
                        rc = lib.mpe_tracker_estimate_batch_device_encoded(tsp, n, enc_ptrs[k], rows, cols, cols * bpp, enc, 0,
                                                                           tk[k].ctypes.data_as(dp), rec[k].ctypes.data,
                                                                           info[k].ctypes.data, None)
                    assert rc >= 0, (way, k, rc, lib.mpe_last_error(h._h).decode())

            def split(h):
                return ({w: round(h.get_option("track_ns_" + w) / 1e3, 2) for w in ("pack", "enqueue", "wait")},
                        h.get_option("track_steps"))

            ms = {"A": [], "B": []}
            cold = {"A": [], "B": []}
            ref = None
            conv_ms = []
            for rep in range(args.reps):
                for way in ("A", "B"):
                    h = mpe.Handle(0)
                    mk = lambda: [mpe.Tracker(h, M, K0, D0, P) for _ in range(n)]
                    ts = mk()
                    run(way, h, ts, WARMUP)
                    for t in ts:
                        t.close()
                    ts = mk()
                    h.set_option("track_profile", 1)
                    t0 = time.perf_counter()
                    run(way, h, ts, steps)
                    dt = time.perf_counter() - t0
                    us, subs = split(h)
                    h.set_option("track_profile", 0)
                    for t in ts:
                        t.close()
                    if ref is None:
                        ref = (rec.tobytes(), info.tobytes())
                    assert (rec.tobytes(), info.tobytes()) == ref, "records of way %s differ (repetition %d)" % (way, rep)
                    ms[way].append(dt * 1e3 / steps)
                    emit(dict(tool="encoded_frame_streams", encoding=encoding, way=way, streams=n, steps=steps, rep=rep,
                              ms_per_step=round(dt * 1e3 / steps, 4), tracked_frames_per_s=round(n * steps / dt, 1),
                              submissions=subs, us_per_submission=us, poses=int((rec["status"] == 0).sum()),
                              brute_force_frames=int(info[:, :, 7].sum())))
                    # the cold start alone: the first time step of fresh trackers, every stream's whole frame submitted
                    t_cold = []
                    for _ in range(COLD_REPS):
                        ts = mk()
                        t0 = time.perf_counter()
                        run(way, h, ts, 1)
                        t_cold.append((time.perf_counter() - t0) * 1e3)
                        for t in ts:
                            t.close()
                    cold[way].append(float(np.median(t_cold)))
                    emit(dict(tool="encoded_frame_streams", encoding=encoding, way=way, streams=n, rep=rep,
                              cold_first_step_ms=round(cold[way][-1], 4), cold_steps_timed=COLD_REPS))
                    if way == "A":   # the conversion of one time step alone, call to completion
                        t_conv = []
                        for k in range(COLD_REPS):
                            h.synchronize()
                            t0 = time.perf_counter()
                            lib.mpe_convert_to_mono8(h._h, C.c_void_p(frames[k].data_ptr()), 1, enc, 0, n, rows, cols,
                                                     C.c_size_t(cols * bpp), C.c_size_t(fbytes), C.c_void_p(mono.data_ptr()), 1)
                            h.synchronize()
                            t_conv.append((time.perf_counter() - t0) * 1e3)
                        conv_ms.append(float(np.median(t_conv)))
                        emit(dict(tool="encoded_frame_streams", encoding=encoding, way=way, streams=n, rep=rep,
                                  convert_launch_ms=round(conv_ms[-1], 4), mb_read=round(n * fbytes / 1e6, 1),
                                  mb_written=round(n * rows * cols / 1e6, 1)))
                    h.close()
            am, bm = np.array(ms["A"]), np.array(ms["B"])
            emit(dict(tool="encoded_frame_streams", summary=True, encoding=encoding, streams=n, steps=steps, reps=args.reps,
                      a_ms_per_step=[round(float(v), 4) for v in am], b_ms_per_step=[round(float(v), 4) for v in bm],
                      a_spread_ms=round(float(am.max() - am.min()), 4),
                      a_minus_b_ms=round(float(np.median(am) - np.median(bm)), 4),
                      b_beats_a_by_more_than_a_spread=bool(np.median(am) - np.median(bm) > am.max() - am.min()),
                      b_over_a=round(float(np.median(bm) / np.median(am)), 3),
                      cold_first_step_a_ms=round(float(np.median(cold["A"])), 4),
                      cold_first_step_b_ms=round(float(np.median(cold["B"])), 4),
                      convert_launch_ms=round(float(np.median(conv_ms)), 4), b_records_equal_a=True))
            del frames, mono, enc_ptrs
            torch.cuda.empty_cache()
        del e_traj
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
