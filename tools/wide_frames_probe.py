"""What a glare frame costs, for the record: wall time of mpe_solve_bruteforce_batch_wide for ONE detection set (65 / 4,
128 / 5, 256 / 5 detections / markers), and of mpe_estimate_batch_wide over 4096 device frames with one wide frame
against mpe_estimate_batch over the same frames; 3 timed calls each behind a warm-up call.
    python tools/wide_frames_probe.py [out.jsonl]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rpg_monocular_pose_estimator_amd as mpe
from rpg_monocular_pose_estimator_amd import synth

K, D = synth.camera_for(480, 752)
h = mpe.Handle()
rng = np.random.default_rng(1)
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
for n_det, markers in ((65, synth.M5[:4]), (128, synth.M5), (256, synth.M5)):
    _, spots = synth.sample_scene(rng, markers, K, D, 480, 752, n_distractors=n_det - len(markers))
    P = mpe.demo_params()
    h.solve_bruteforce_batch_wide([spots], markers, K, P)  # (warm-up: buffers, code objects)
    ms = []
    for _ in range(3):
        t = time.perf_counter()
        rec, _, _ = h.solve_bruteforce_batch_wide([spots], markers, K, P)
        ms.append((time.perf_counter() - t) * 1e3)
    n_m = len(markers)
    hyp = n_det * (n_det - 1) * (n_det - 2) // 6 * n_m * (n_m - 1) * (n_m - 2)
    out.write(json.dumps(dict(entry="mpe_solve_bruteforce_batch_wide", items=1, n_det=n_det, n_markers=n_m, hypotheses=hyp,
                              wall_ms=[round(v, 3) for v in ms], status=int(rec["status"][0]))) + "\n")
    out.flush()
h.close()

# mpe_estimate_batch_wide over 4096 device frames of which ONE is wide (70 spots), against mpe_estimate_batch over the same
import torch
h = mpe.Handle()
base = synth.make_frames("C2", 64, seed=5)
frames = np.ascontiguousarray(np.tile(base["frames"], (64, 1, 1)))
rng = np.random.default_rng(2)
_, spots = synth.sample_scene(rng, synth.M5, K, D, 480, 752, n_distractors=65)
frames[1000] = synth.render_frame(rng, spots, 480, 752)
d = torch.from_numpy(frames).cuda()
P = mpe.demo_params()
for name, fn in (("mpe_estimate_batch", h.estimate_batch), ("mpe_estimate_batch_wide", h.estimate_batch_wide)):
    fn(d, synth.M5, K, D, P)
    ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        rec = fn(d, synth.M5, K, D, P)
        ms.append((time.perf_counter() - t) * 1e3)
    out.write(json.dumps(dict(entry=name, frames=4096, wide_frames=1, wide_n_det=int(rec["n_det"][1000]),
                              wide_status=int(rec["status"][1000]), wall_ms=[round(v, 3) for v in ms])) + "\n")
    out.flush()
h.close()
