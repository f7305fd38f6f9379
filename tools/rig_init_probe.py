"""What finding a body with the whole rig costs, for the record (recorded, not gated): mpe_rig_init_batch over 1, 64 and
4096 problems of the [3, 3, 2] kind (three cameras, five markers, 0.1 px noise) with 2 and with 8 stray detections per
camera — 1 440 and 27 000 items a problem.  Timed with HIP events (option "rig_launch_profile": a pair of events around
the call's four launches, the copies outside), the median of 7 calls behind a warm-up call, and the wall time of the whole
call beside it.  The only comparison that exists is the host tier: the same header compiled with g++ -O2
(tests/host/rig_init_host.cpp), one core, over the first problems of the batch.  All configurations run in ONE child
process under one time limit; a failure ends the tool.  One line per configuration is appended to the file.
    python tools/rig_init_probe.py [profiles/rig_init.jsonl]"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BATCHES = (1, 64, 4096)
STRAY = (2, 8)
HOST_PROBLEMS = 8                 # problems the host tier is timed over
LIMIT = 420                       # seconds for the whole run


def measure():
    import numpy as np
    import rpg_monocular_pose_estimator_amd as mpe
    import test_rig_init_host as TH
    import witness_rig
    import witness_rig_init as WI
    host = TH.build_host(tempfile.mkdtemp(prefix="rig_init_probe"))
    h = mpe.Handle()
    h.set_option("rig_launch_profile", 1)
    for stray in STRAY:
        rng = np.random.default_rng(100 + stray)
        rig = (witness_rig.random_cameras(rng, 3), rng.uniform(-0.25, 0.25, (5, 3)))
        items = [WI.random_problem(rng, [3, 3, 2], clutter=stray, rig=rig)[0] for _ in range(max(BATCHES))]
        t0 = time.perf_counter()
        host_reasons = [int(TH.host_init(host, p)[2]["reason"]) for p in items[:HOST_PROBLEMS]]
        host_us = (time.perf_counter() - t0) / HOST_PROBLEMS * 1e6
        for n in BATCHES:
            dets = [p[2] for p in items[:n]]

            def call():
                return h.rig_init_batch(rig[0], rig[1], dets, 3.0, 3.0)
            rec, match, info = call()
            assert [int(r) for r in info["reason"][:HOST_PROBLEMS]] == host_reasons[:n]
            ns, wall = [], []
            for _ in range(7):
                t0 = time.perf_counter()
                call()
                wall.append(time.perf_counter() - t0)
                ns.append(h.get_option("rig_launch_ns"))
            dev_us, n_it = float(np.median(ns)) / 1e3, int(info["n_items"].sum())
            print(json.dumps(dict(
                kind=[3, 3, 2], stray_per_camera=stray, problems=n, items_per_problem=round(n_it / n), poses=int((rec["status"] == 0).sum()),
                ambiguous=int((info["reason"] == 5).sum()), launches_us=round(dev_us, 1), us_per_launch=round(dev_us / 4, 1),
                call_us=round(float(np.median(wall)) * 1e6, 1), problems_per_s=round(n / dev_us * 1e6), items_per_s=round(n_it / dev_us * 1e6),
                host_one_core_us_per_problem=round(host_us, 1), host_items_per_s=round(n_it / n / host_us * 1e6))), flush=True)
    h.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--measure":
        measure()
        sys.exit(0)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure"], capture_output=True, text=True, timeout=LIMIT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit("the measurement failed with %d" % r.returncode)
    out = open(sys.argv[1], "a") if len(sys.argv) > 1 else sys.stdout
    out.write(r.stdout)
