"""What the marker calibration costs and gives, for the record (recorded, not gated): mpe_body_calibrate over synthetic
recordings of (1 camera, 5 markers, 100 views) and (3 cameras, 5 markers, 1000 views), start markers 4 mm off — the
iteration count, the shape error before and after (largest marker distance after a rigid alignment; a similarity when
scale is held), the device time per iteration split by step (option "rig_ba_profile": events around every launch), the
launches and the wall time of the whole call (input packing in numpy not included) —, and a rendered sequence through
BodyCalibrator (2 cameras, 5 markers about 3 mm off, 40 frames: the trackers' own correspondences and detections).
Every configuration runs in a child process of its own under its own time limit; a configuration that fails or runs out
of time ends the tool.
    python tools/body_calibration_numbers.py [profiles/body_calibration.jsonl]"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = [(1, 5, 100, 120), (3, 5, 1000, 120)]   # cameras, markers, views, time limit [s]
STEPS = ("linearise", "reduce", "solve", "update", "finish", "covariance")


def one(n_cam, n_markers, n_views):
    import numpy as np
    import rpg_monocular_pose_estimator_amd as mpe
    import witness_body_ba as wbb
    prob = wbb.random_body_calibration(np.random.default_rng(3), n_cam, n_views, n_markers, p_missing=0.1)
    cams, begin, cam, mk_idx, uv = mpe.pack_body_views(prob["cameras"], prob["views"])
    mk = np.ascontiguousarray(prob["markers"], float)
    T0 = np.ascontiguousarray(prob["T_start"], float).reshape(-1, 16)
    h = mpe.Handle()
    lib = h._lib
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    P, T_out, cov = np.zeros((n_markers, 3)), np.zeros((n_views, 4, 4)), np.zeros((n_markers, 3, 3))
    rep = mpe.MpeBodyCalibrationReport()

    def call():
        t = time.perf_counter()
        rc = lib.mpe_body_calibrate(h._h, cams, n_cam, mk.ctypes.data_as(dp), n_markers, begin.ctypes.data_as(ip),
                                    cam.ctypes.data_as(ip), mk_idx.ctypes.data_as(ip), uv.ctypes.data_as(dp), n_views,
                                    T0.ctypes.data_as(dp), None, P.ctypes.data_as(dp), T_out.ctypes.data_as(dp),
                                    cov.ctypes.data_as(dp), None, C.byref(rep))
        assert rc == 1, (rc, lib.mpe_last_error(h._h).decode())
        return (time.perf_counter() - t) * 1e3
    call()                                                # (buffers allocated, kernels loaded)
    wall = sorted(call() for _ in range(3))
    h.set_option("rig_ba_profile", 1)
    call()
    us = {s: h.get_option("body_ba_us_" + s) for s in STEPS}
    launches = h.get_option("body_ba_launches")
    it = rep.iterations
    held = bool(rep.scale_held)
    # (one chunk: the linearisation runs once per iteration and once more behind the last one, for the final residuals)
    per_it = {s: round(us[s] / 1e3 / it, 4) for s in STEPS[:5]}
    per_it["linearise"] = round(us["linearise"] / 1e3 / (it + 1), 4)
    print(json.dumps(dict(
        entry="mpe_body_calibrate", cameras=n_cam, markers=n_markers, views=n_views, rows=int(rep.rows_used), iterations=it,
        scale_held=int(held), rms_before=round(rep.rms_before, 4), rms_after=round(rep.rms_after, 4), last_step=rep.last_step,
        shape_error_before_m=wbb.shape_error(prob["markers"], prob["markers_true"], held),
        shape_error_after_m=wbb.shape_error(P, prob["markers_true"], held),
        sigma_mm_per_pixel_worst=float(np.sqrt(max(cov[m].diagonal().max() for m in range(n_markers))) * 1e3),
        launches=launches, ms_per_iteration_by_step=per_it,
        device_ms_by_step={s: round(us[s] / 1e3, 3) for s in STEPS}, device_ms_total=round(sum(us.values()) / 1e3, 3),
        wall_ms_median=round(wall[1], 3), wall_ms_min=round(wall[0], 3))))
    h.close()


def rendered():
    import numpy as np
    import rpg_monocular_pose_estimator_amd as mpe
    from rpg_monocular_pose_estimator_amd import synth
    import witness_body_ba as wbb
    K0, D0 = synth.camera_for(480, 752)
    E1 = np.eye(4)
    E1[:3, :3] = synth.rodrigues([0.1, 1.0, 0.05], -0.04)
    E1[:3, 3] = [-0.06, 0.01, 0.005]
    cams, E = [(K0, D0), (K0 * np.array([[1.02], [0.985], [1.0]]), D0 * 0.9)], np.array([np.eye(4), E1])
    nominal = np.asarray(synth.CONFIGS["C2"]["markers"], float)
    truth = nominal + np.random.default_rng(50).normal(size=nominal.shape) * 0.003 / np.sqrt(3)
    seq = synth.make_rig_sequence("C2", 40, 5, cams, E, ang_speed=1.2, true_markers=truth)
    h = mpe.Handle()
    trackers = [mpe.Tracker(h, seq["markers"], K, D, mpe.demo_params()) for K, D in cams]
    cal = mpe.BodyCalibrator(h, trackers, E)
    for k in range(40):
        cal.step([f[k] for f in seq["frames"]], [seq["times"][k]] * 2)
    out = cal.solve()
    rep = out["report"]
    assert out["ok"], rep
    print(json.dumps(dict(
        entry="BodyCalibrator", what="rendered sequence, 2 cameras x 5 markers x 40 frames, markers 3 mm off",
        views_used=rep["views_used"], rows_used=rep["rows_used"], iterations=rep["iterations"], scale_held=rep["scale_held"],
        rms_before=round(rep["rms_before"], 4), rms_after=round(rep["rms_after"], 4),
        shape_error_before_m=wbb.shape_error(nominal, truth, False), shape_error_after_m=wbb.shape_error(out["markers"], truth, False))))
    for t in trackers:
        t.close()
    h.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--rendered":
        rendered()
        sys.exit(0)
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    jobs = [(["--one", str(c), str(m), str(v)], limit) for c, m, v, limit in CONFIGS] + [(["--rendered"], 120)]
    for args, limit in jobs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("configuration %s failed with %d: nothing more is started" % (" ".join(args), r.returncode))
        out.write(r.stdout.strip().splitlines()[-1] + "\n")
        out.flush()
