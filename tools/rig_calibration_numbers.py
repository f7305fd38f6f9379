"""What the rig calibration costs, for the record (recorded, not gated): mpe_rig_calibrate over synthetic recordings of
(3 cameras, 4 096 views, 5 markers) and (16 cameras, 16 384 views, 16 markers) — the iteration count, the device time
per iteration split by step (option "rig_ba_profile": events around every launch), the launches, the chunks the views'
records were worked through in, and the wall time of the whole call (input packing in numpy not included: the arrays are
packed once).  Every configuration runs in a child process of its own under its own time limit; a configuration that
fails or runs out of time ends the tool.
    python tools/rig_calibration_numbers.py [profiles/rig_calibration.jsonl]"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [(3, 4096, 5, 120), (16, 16384, 16, 400)]   # cameras, views, markers, time limit [s]
STEPS = ("linearise", "reduce", "solve", "update", "finish", "covariance")


def recording(n_cam, n_views, n_markers, seed=3):
    """Every camera sees every marker in every view (0.1 px noise); start values 0.03 rad / 0.01 m (extrinsics) and
    0.05 rad / 0.01 m (poses) off, packed as mpe_rig_calibrate takes them."""
    import numpy as np
    from rpg_monocular_pose_estimator_amd import synth
    rng = np.random.default_rng(seed)

    def rigid(angle, shift):
        T = np.eye(4)
        T[:3, :3] = synth.rodrigues(rng.normal(size=3), angle)
        T[:3, 3] = shift
        return T
    markers = rng.uniform(-0.25, 0.25, (n_markers, 3))
    K = np.array([[rng.uniform(400, 460, n_cam), np.zeros(n_cam), rng.uniform(360, 390, n_cam)],
                  [np.zeros(n_cam), rng.uniform(400, 460, n_cam), rng.uniform(230, 250, n_cam)],
                  [np.zeros(n_cam), np.zeros(n_cam), np.ones(n_cam)]]).transpose(2, 0, 1)
    E = np.array([rigid(rng.uniform(0, 0.5), rng.uniform(-0.3, 0.3, 3)) for _ in range(n_cam)])
    T = np.array([rigid(rng.uniform(0, 0.6), [rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(1.2, 2.2)])
                  for _ in range(n_views)])
    X = np.einsum("fij,mj->fmi", T[:, :3, :3], markers) + T[:, None, :3, 3]            # (views, markers, 3)
    q = np.einsum("cij,fmj->fcmi", E[:, :3, :3], X) + E[None, :, None, :3, 3]           # (views, cameras, markers, 3)
    uv = np.stack([K[None, :, None, 0, 0] * q[..., 0] / q[..., 2] + K[None, :, None, 0, 2],
                   K[None, :, None, 1, 1] * q[..., 1] / q[..., 2] + K[None, :, None, 1, 2]], -1)
    uv = (uv + rng.normal(0, 0.1, uv.shape)).astype(np.float32).astype(np.float64)
    per = n_cam * n_markers
    begin = (np.arange(n_views + 1) * per).astype(np.int32)
    cam = np.ascontiguousarray(np.tile(np.repeat(np.arange(n_cam, dtype=np.int32), n_markers), n_views))
    xyz = np.ascontiguousarray(np.tile(markers, (n_views * n_cam, 1)))
    E0 = np.array([E[c] if c == 0 else rigid(0.03, rng.normal(size=3) * 0.01 / np.sqrt(3)) @ E[c] for c in range(n_cam)])
    T0 = np.ascontiguousarray([rigid(0.05, rng.normal(size=3) * 0.01 / np.sqrt(3)) @ Tf for Tf in T])
    return K, E, E0, begin, cam, xyz, np.ascontiguousarray(uv.reshape(-1, 2)), T0


def one(n_cam, n_views, n_markers):
    import numpy as np
    import rpg_monocular_pose_estimator_amd as mpe
    K, E, E0, begin, cam, xyz, uv, T0 = recording(n_cam, n_views, n_markers)
    h = mpe.Handle()
    lib = h._lib
    cams = (mpe.MpeRigCamera * n_cam)()
    for c in range(n_cam):
        cams[c].K[:] = K[c].reshape(9)
        cams[c].T_cam_rig[:] = E0[c].reshape(16)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    E_out, T_out, cov = np.zeros((n_cam, 4, 4)), np.zeros((n_views, 4, 4)), np.zeros((n_cam, 6, 6))
    rep = mpe.MpeRigCalibrationReport()

    def call():
        t = time.perf_counter()
        rc = lib.mpe_rig_calibrate(h._h, cams, n_cam, begin.ctypes.data_as(ip), cam.ctypes.data_as(ip), xyz.ctypes.data_as(dp),
                                   uv.ctypes.data_as(dp), n_views, T0.ctypes.data_as(dp), None, E_out.ctypes.data_as(dp),
                                   T_out.ctypes.data_as(dp), cov.ctypes.data_as(dp), None, C.byref(rep))
        assert rc == 1, (rc, lib.mpe_last_error(h._h).decode())
        return (time.perf_counter() - t) * 1e3
    call()                                                # (buffers allocated, kernels loaded)
    wall = sorted(call() for _ in range(3))
    h.set_option("rig_ba_profile", 1)
    call()
    us = {s: h.get_option("rig_ba_us_" + s) for s in STEPS}
    launches = h.get_option("rig_ba_launches")
    it = rep.iterations
    slots = n_cam - 1
    rec_bytes = n_views * (8 + 99 * slots) * 8
    chunks = -(-rec_bytes // (65536 * 1024))
    # (the linearisation runs once more behind the last iteration — the residuals at the final values — and, with more
    #  than one chunk, a second time per iteration in front of the update: its share per iteration leaves that last pass out)
    n_lin = (2 * it + 1) if chunks > 1 else it + 1
    per_it = {s: round(us[s] / 1e3 / it, 4) for s in STEPS[:5]}
    per_it["linearise"] = round(us["linearise"] / 1e3 * (n_lin - 1) / n_lin / it, 4)
    print(json.dumps(dict(
        entry="mpe_rig_calibrate", cameras=n_cam, views=n_views, markers=n_markers, rows=int(len(cam)), iterations=it,
        rms_before=round(rep.rms_before, 4), rms_after=round(rep.rms_after, 4), last_step=rep.last_step,
        worst_extrinsic_entry_error=float(np.abs(E_out - E).max()), record_bytes=rec_bytes, chunks=int(chunks),
        launches=launches, ms_per_iteration_by_step=per_it, linearisations=n_lin,
        device_ms_by_step={s: round(us[s] / 1e3, 3) for s in STEPS}, device_ms_total=round(sum(us.values()) / 1e3, 3),
        wall_ms_median=round(wall[1], 3), wall_ms_min=round(wall[0], 3))))
    h.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
        sys.exit(0)
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    for n_cam, n_views, n_markers, limit in CONFIGS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n_cam), str(n_views), str(n_markers)],
                           capture_output=True, text=True, timeout=limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("configuration (%d, %d, %d) failed with %d: nothing more is started" % (n_cam, n_views, n_markers, r.returncode))
        out.write(r.stdout.strip().splitlines()[-1] + "\n")
        out.flush()
