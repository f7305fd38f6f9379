"""What the rig fusion costs, for the record (recorded, not gated): wall time of mpe_rig_optimise_pose_batch for ONE problem
of 4 cameras x 5 rows per call beside mpe_optimise_pose on one camera's 5 rows; one call of 4 096 such problems; and a
lock-step time step of a 4-camera rig with and without the fusion (Rig.step against tracker_estimate_batch_mixed over
the same frames).  Both C entries are called through ctypes on arrays packed once.
    python tools/rig_fusion_numbers.py [profiles/rig_fusion.jsonl]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rpg_monocular_pose_estimator_amd as mpe
from rpg_monocular_pose_estimator_amd import synth

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def emit(**kw):
    out.write(json.dumps(kw) + "\n")
    out.flush()


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return dict(calls=len(ms), median_ms=round(float(np.median(ms)), 4), min_ms=round(float(ms[0]), 4),
                p90_ms=round(float(ms[int(0.9 * (len(ms) - 1))]), 4))


def rig_cameras(n):
    """n cameras of C2's image size on a short base line, camera 0 the rig frame."""
    K0, D0 = synth.camera_for(480, 752)
    cams, E = [], []
    for c in range(n):
        K = K0.copy()
        K[0, 0] *= 1.0 + 0.02 * c
        K[1, 1] *= 1.0 - 0.015 * c
        cams.append((K, D0.copy()))
        T = np.eye(4)
        if c:
            T[:3, :3] = synth.rodrigues([0.1, 1.0, 0.05 * c], 0.03 * c * (-1) ** c)
            T[:3, 3] = [0.05 * c * (-1) ** c, 0.01 * c, 0.0]
        E.append(T)
    return cams, np.array(E)


h = mpe.Handle()
lib = h._lib
cams, E = rig_cameras(4)
rng = np.random.default_rng(3)
markers = np.asarray(synth.M5, float)
T_true = np.eye(4)
T_true[:3, :3] = synth.rodrigues([0.3, 1.0, 0.2], 0.4)
T_true[:3, 3] = [0.05, -0.03, 1.6]
rows_cam, rows_xyz, rows_uv = [], [], []
for c, (K, _) in enumerate(cams):
    px = synth.project(E[c] @ T_true, markers, K) + rng.normal(0, 0.1, (5, 2))
    rows_cam += [c] * 5
    rows_xyz.append(markers)
    rows_uv.append(px)
T0 = T_true.copy()
T0[:3, :3] = synth.rodrigues([1.0, 0.2, 0.1], 0.05) @ T0[:3, :3]
T0[:3, 3] += 0.006

rc_cams = (mpe.MpeRigCamera * 4)()
for c, (K, _) in enumerate(cams):
    rc_cams[c].K[:] = K.reshape(9)
    rc_cams[c].T_cam_rig[:] = E[c].reshape(16)


def rig_call(n):
    begin = np.arange(n + 1, dtype=np.int32) * 20
    cam = np.tile(np.asarray(rows_cam, np.int32), n)
    xyz = np.ascontiguousarray(np.tile(np.vstack(rows_xyz), (n, 1)))
    uv = np.ascontiguousarray(np.tile(np.vstack(rows_uv), (n, 1)))
    t0 = np.ascontiguousarray(np.tile(T0.reshape(16), (n, 1)))
    rec = np.zeros(n, mpe.RESULT_DTYPE)

    def call():
        rc = lib.mpe_rig_optimise_pose_batch(h._h, rc_cams, 4, begin.ctypes.data_as(ip), cam.ctypes.data_as(ip),
                                             xyz.ctypes.data_as(dp), uv.ctypes.data_as(dp), n, t0.ctypes.data_as(dp),
                                             rec.ctypes.data)
        assert rc == 0, rc
        return rec
    return call


def timed(call, n_calls, warm=20):
    for _ in range(warm):
        call()
    ms = []
    for _ in range(n_calls):
        t = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t) * 1e3)
    return ms


one = rig_call(1)
rec = one()
emit(entry="mpe_rig_optimise_pose_batch", problems=1, cameras=4, rows=20, gn_iterations=int(rec["gn_iterations"][0]),
     status=int(rec["status"][0]), **stats(timed(one, 300)))

# mpe_optimise_pose on camera 0's five rows, same box, same start (camera 0 is the rig frame)
K0 = np.ascontiguousarray(cams[0][0].reshape(9))
det = np.ascontiguousarray(rows_uv[0])
corr = np.ascontiguousarray(np.column_stack([np.arange(1, 6), np.arange(1, 6)]), np.uint32)
P = mpe.demo_params()
res = mpe.MpeResult()
t0_one = np.ascontiguousarray(T0.reshape(16))


def single():
    rc = lib.mpe_optimise_pose(h._h, det.ctypes.data_as(dp), 5, markers.ctypes.data_as(dp), 5, K0.ctypes.data_as(dp),
                               C.byref(P), corr.ctypes.data_as(C.POINTER(C.c_uint32)), 5, t0_one.ctypes.data_as(dp),
                               C.byref(res))
    assert rc == 0, rc


single()
emit(entry="mpe_optimise_pose", problems=1, cameras=1, rows=5, gn_iterations=int(res.gn_iterations), status=int(res.status),
     **stats(timed(single, 300)))

many = rig_call(4096)
rec = many()
assert (rec["status"] == 0).all() and np.array_equal(rec["T"][0], rec["T"][4095])
emit(entry="mpe_rig_optimise_pose_batch", problems=4096, cameras=4, rows=20, gn_iterations=int(rec["gn_iterations"][0]),
     **stats(timed(many, 30, warm=5)))

# a lock-step time step of the 4-camera rig, with and without the fusion: three alternating repetitions of a 64-frame replay
seq = synth.make_rig_sequence("C2", 64, 5, cams, E)
P = mpe.demo_params()
for rep in range(3):
    for fusion in (False, True):
        ts = [mpe.Tracker(h, seq["markers"], K, D, P) for K, D in cams]
        rig = mpe.Rig(h, ts, E)
        ms, fused_n = [], 0
        for k in range(64):
            imgs = [f[k] for f in seq["frames"]]
            times = [seq["times"][k]] * 4
            t = time.perf_counter()
            if fusion:
                fused_n += int(rig.step(imgs, times)[4])
            else:
                mpe.tracker_estimate_batch_mixed(ts, imgs, times)
            ms.append((time.perf_counter() - t) * 1e3)
        emit(entry="Rig.step" if fusion else "tracker_estimate_batch_mixed", streams=4, frames=64, repetition=rep,
             fused_steps=fused_n, **stats(ms[4:]))
        for t in ts:
            t.close()
h.close()
