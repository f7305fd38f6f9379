"""mpe_solve_bruteforce_batch_setups alone: the fused call against the per-set-up loop of mpe_solve_bruteforce_batch
in the same process, host clock around the blocking calls, after warm-up.  Two shapes by default:

  64 set-ups x 1 item of 5 detections / 5 markers   (the start of 64 cameras: launch chains dominate the loop)
   8 set-ups x 8 items of 12 detections / 8 markers (73 920 hypotheses per item: the strict loop nest's cost shows)

One JSON line per shape: microseconds per call (median and quartiles over --reps calls) of both ways and their ratio;
the records of the two ways must be equal byte for byte (asserted).

    python tools/bruteforce_setups_probe.py [--shapes 64x1x5x5,8x8x12x8] [--reps 50] [--out FILE]
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

WARMUP = 5
ROWS, COLS = 480, 752


def camera_of(j, K, D):
    K = K.copy()
    K[0, 0] *= 1.0 + 3e-4 * j
    K[1, 1] *= 1.0 + 2e-4 * j
    K[0, 2] += 0.01 * j
    K[1, 2] -= 0.01 * j
    return K, D.copy()


def markers_of(n_markers):
    base = {4: synth.M4, 5: synth.M5, 8: synth.M8}
    if n_markers in base:
        return base[n_markers]
    rng = np.random.default_rng(n_markers)
    return np.vstack([synth.M8, rng.uniform(-0.09, 0.09, (n_markers - 8, 3))])[:n_markers]


def quartiles(us):
    q = np.percentile(us, [25, 50, 75])
    return dict(q25=round(float(q[0]), 1), median=round(float(q[1]), 1), q75=round(float(q[2]), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x1x5x5,8x8x12x8", help="set-ups x items per set-up x detections x markers")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    K0, D0 = synth.camera_for(ROWS, COLS)
    h = mpe.Handle(0)
    lines = []
    for shape in args.shapes.split(","):
        n_su, per, n_det, n_m = [int(x) for x in shape.split("x")]
        M = markers_of(n_m)
        P = mpe.demo_params(back_projection_pixel_tolerance=2.0 if n_m >= 8 else 5.0)
        setups = [(M,) + camera_of(j, K0, D0) + (P,) for j in range(n_su)]
        dets, item_setup = [], []
        for i in range(n_su * per):
            s = i % n_su
            rng = np.random.default_rng([77, i])
            T, spots = synth.sample_scene(rng, M, setups[s][1], D0, ROWS, COLS, max(0, n_det - n_m))
            px = np.vstack([synth.project(T, M, setups[s][1]), spots[len(M):]])[:n_det]
            dets.append(px)
            item_setup.append(s)
        by_setup = [[i for i in range(len(dets)) if item_setup[i] == s] for s in range(n_su)]

        def fused():
            return h.solve_bruteforce_batch_setups(dets, setups, item_setup)

        def loop():
            rec = np.zeros(len(dets), mpe.RESULT_DTYPE)
            for s, idx in enumerate(by_setup):
                r, _, _ = h.solve_bruteforce_batch([dets[i] for i in idx], M, setups[s][1], P)
                rec[idx] = r
            return rec

        c0 = h.get_option("bruteforce_submits")
        ref_f = fused()[0]
        c1 = h.get_option("bruteforce_submits")
        ref_l = loop()
        c2 = h.get_option("bruteforce_submits")
        assert ref_f.tobytes() == ref_l.tobytes(), "fused call and per-set-up loop differ"
        t = {"fused": [], "loop": []}
        for k in range(WARMUP + args.reps):
            for name, fn in (("fused", fused), ("loop", loop)):   # alternating: both see the same clocks and caches
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if k >= WARMUP:
                    t[name].append(dt * 1e6)
        line = dict(tool="bruteforce_setups_probe", setups=n_su, items=len(dets), detections=n_det, markers=n_m,
                    hypotheses_per_item=n_det * (n_det - 1) * (n_det - 2) // 6 * n_m * (n_m - 1) * (n_m - 2),
                    submits_fused=c1 - c0, submits_loop=c2 - c1, poses=int((ref_f["status"] == 0).sum()), reps=args.reps,
                    fused_us=quartiles(t["fused"]), loop_us=quartiles(t["loop"]),
                    loop_over_fused=round(float(np.median(t["loop"]) / np.median(t["fused"])), 3))
        s = json.dumps(line)
        print(s, flush=True)
        lines.append(s)
    h.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
