"""What a glare lane costs a lock-step group, for the record: wall time of ONE time step of 1 / 8 / 64 streams
(mpe_tracker_estimate_batch_mixed, trackers with mpe_tracker_set_wide_frames on) in which stream 0
  roi_glare : is tracked through a ROI of 107 detections (frame 3 of a C1 sequence, 103 rectangles painted into its ROI),
  init_glare: initialises over 70 detections (frame 0 with 66 rectangles; every stream initialises on that step),
against the same step with stream 0 on the clean frame.  Every repetition runs fresh trackers up to the timed step;
3 timed repetitions behind a warm-up one.
    python tools/wide_tracking_probe.py [out.jsonl]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rpg_monocular_pose_estimator_amd as mpe
from rpg_monocular_pose_estimator_amd import synth

BORDER = 45


def paint(img, box, leds, keep, limit=None):
    """4 x 5 rectangles of value 220 on a 12 x 11 pitch, every cell 3 px inside box, `keep` px away from the LEDs"""
    x0, y0, w, h = box
    n = 0
    for y in range(y0 + 3, y0 + h - 3 - 11 + 1, 11):
        for x in range(x0 + 3, x0 + w - 3 - 12 + 1, 12):
            if np.linalg.norm(leds - np.array([x + 2.0, y + 1.5]), axis=1).min() <= keep or (limit is not None and n >= limit):
                continue
            img[y:y + 4, x:x + 5] = 220
            n += 1
    return n


d = synth.make_sequence("C1", 6, 3)
leds = lambda k: synth.distort_px(synth.project(d["T_true"][k], d["markers"], d["K"]), d["K"], d["D"])
P = mpe.demo_params(roi_border_thickness=BORDER)
h = mpe.Handle()


def trackers(n):
    ts = [mpe.Tracker(h, d["markers"], d["K"], d["D"], P) for _ in range(n)]
    for t in ts:
        t.set_wide_frames(True)
    return ts


# the ROI of frame 3 follows from frames 0 .. 2: read it off a clean run
t0 = trackers(1)[0]
roi3 = [t0.estimate(d["frames"][k], d["times"][k]) for k in range(4)][3]["roi"]
t0.close()
glare3 = d["frames"][3].copy()
paint(glare3, roi3, leds(3), 14.0)
glare0 = d["frames"][0].copy()
paint(glare0, (197, 57, 406, 336), leds(0), 40.0, limit=66)
CASES = (("roi_glare", 3, glare3), ("init_glare", 0, glare0))

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
for case, step, glare in CASES:
    for n in (1, 8, 64):
        ms = {"clean": [], "glare": []}
        seen = {}
        for rep in range(4):
            for kind in ("clean", "glare"):
                ts = trackers(n)
                for k in range(step):
                    mpe.tracker_estimate_batch_mixed(ts, [d["frames"][k]] * n, [d["times"][k]] * n)
                imgs = [glare if kind == "glare" else d["frames"][step]] + [d["frames"][step]] * (n - 1)
                c0 = h.get_option("wide_track_submits")
                t = time.perf_counter()
                rec, info, upd = mpe.tracker_estimate_batch_mixed(ts, imgs, [d["times"][step]] * n)
                dt = (time.perf_counter() - t) * 1e3
                if rep:  # (repetition 0 warms up)
                    ms[kind].append(round(dt, 3))
                seen[kind] = dict(n_det=int(info[0, 5]), status=int(rec["status"][0]), used_bruteforce=int(info[0, 7]),
                                  wide_track_submits=h.get_option("wide_track_submits") - c0)
                for t_ in ts:
                    t_.close()
        out.write(json.dumps(dict(case=case, streams=n, step=step, clean_ms=ms["clean"], glare_ms=ms["glare"],
                                  clean=seen["clean"], glare=seen["glare"])) + "\n")
        out.flush()
h.close()
