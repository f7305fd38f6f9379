"""Informational numbers for the Bayer / YUV 4:2:2 encodings (profiles/sensor_encodings.jsonl).

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o s -- python tools/sensor_encoding_numbers.py gather
      30 time steps each of 64 streams with ROIs of 120 x 120 in bgr8, bayer_rggb8 and yuv422 through
      track_step_batch_device(..., encoding=...); the gather launches' times are read off OUT/s_kernel_stats.csv
  python tools/sensor_encoding_numbers.py convert
      mpe_convert_to_mono8 over 2048 device frames of 752 x 480 as mono8 (a copy) and as bayer_rggb8: wall clock around
      call + synchronisation, median of 10, as a fraction of the bytes moved (read + written) over the time"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import rpg_monocular_pose_estimator_amd as mpe
from rpg_monocular_pose_estimator_amd import synth
import witness_sensor_encodings as wit

mode = sys.argv[1]
h = mpe.Handle(0)
if mode == "gather":
    scenes = [synth.make_sequence("C2", 1, seed=4000 + s) for s in range(4)]
    q0 = scenes[0]
    rows, cols = int(q0["rows"]), int(q0["cols"])
    setups = [(q0["markers"], q0["K"], q0["D"], mpe.demo_params())]
    rois, preds, which = [], [], []
    for i in range(64):
        q = scenes[i % 4]
        pred = synth.project(q["T_true"][0], q["markers"], q["K"])
        px = synth.distort_px(pred, q["K"], q["D"])
        cx, cy = px.mean(0)
        x0 = int(min(max(cx - 60, 0), cols - 120)) | (i & 1)
        y0 = int(min(max(cy - 60, 0), rows - 120))
        x0 = min(x0, cols - 120)
        rois.append((x0, y0, 120, 120))
        preds.append(pred)
        which.append(i % 4)
    bgr = lambda f: np.ascontiguousarray(np.repeat(f[..., None], 3, axis=-1))
    for enc in ("bgr8", "bayer_rggb8", "yuv422"):
        frames = [torch.from_numpy(bgr(q["frames"][0]) if enc == "bgr8" else wit.mosaic(q["frames"][0], enc, 5)).cuda() for q in scenes]
        imgs = [frames[w] for w in which]
        for it in range(30):
            dets, corr, res = h.track_step_batch_device(imgs, rois, preds, setups, None, encoding=enc)
        print(enc, "status 0:", int((res["status"] == 0).sum()), "of 64", flush=True)
else:
    n, rows, cols = 2048, 480, 752
    g = torch.randint(0, 256, (n, rows, cols), dtype=torch.uint8, device="cuda")
    lib = mpe.load_library()
    import ctypes as C
    dst = torch.empty_like(g)
    def run(enc):
        rc = lib.mpe_convert_to_mono8(h._h, C.c_void_p(g.data_ptr()), 1, enc, 0, n, rows, cols, C.c_size_t(cols), C.c_size_t(rows * cols),
                                      C.c_void_p(dst.data_ptr()), 1)
        assert rc == 0
        h.synchronize()
    out = {}
    for name, enc in (("mono8", 0), ("bayer_rggb8", 16)):
        for _ in range(3):
            run(enc)
        ts = []
        for _ in range(10):
            t0 = time.perf_counter()
            run(enc)
            ts.append(time.perf_counter() - t0)
        t = float(np.median(ts))
        moved = 2.0 * n * rows * cols
        out[name] = dict(ms=t * 1e3, gb_per_s=moved / t / 1e9, frac_of_8tb_s=moved / t / 8e12)
    ref = wit.to_mono8(g[:2].cpu().numpy(), "bayer_rggb8")
    assert np.array_equal(dst[:2].cpu().numpy(), ref)
    print(json.dumps(dict(what="convert_to_mono8 2048 x 752x480, wall clock around call + sync, median of 10", **out)), flush=True)
h.close()
