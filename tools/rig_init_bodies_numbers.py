"""What finding several bodies in one frame costs (mpe_rig_init_bodies_batch), beside the parent's way of doing it: one
mpe_rig_init_batch call per body with the lists filtered on the host in between.  {1, 1 024} problems of 2 x M5 + 4 stray
points and of 4 x M5 + 8 stray points in front of one camera, three repetitions each after one warm-up call; wall time of
the call(s) as the caller sees it (binding included, on both sides).  Appends one JSON line per take.

    python tools/rig_init_bodies_numbers.py profiles/rig_init_bodies.jsonl"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rpg_monocular_pose_estimator_amd as mpe  # noqa: E402
from rpg_monocular_pose_estimator_amd import synth  # noqa: E402

K = synth.camera_for(480, 752)[0]


def scene(rng, n_bodies, strays, min_sep=12.0, noise=0.1):
    """n_bodies M5 bodies at random poses in front of the pinhole camera K plus stray points, every blob at least min_sep
    px from every other and inside 752 x 480, 0.1 px noise, shuffled -> (n, 2)"""
    pts = np.zeros((0, 2))

    def apart(p):
        return (len(pts) == 0 or np.linalg.norm(pts - p, axis=1).min() >= min_sep) and 8 <= p[0] <= 744 and 8 <= p[1] <= 472

    for _ in range(n_bodies):
        while True:
            T = np.eye(4)
            T[:3, :3] = synth.rodrigues(rng.normal(size=3), rng.uniform(0.0, 0.8))
            T[:3, 3] = [rng.uniform(-0.45, 0.45), rng.uniform(-0.3, 0.3), rng.uniform(1.0, 2.0)]
            px = synth.project(T, synth.M5, K) + rng.normal(0, noise, (5, 2))
            d = np.linalg.norm(px[:, None] - px[None], axis=-1) + np.eye(5) * 1e9
            if d.min() >= min_sep and all(apart(p) for p in px):
                break
        pts = np.vstack([pts, px])
    for _ in range(strays):
        while True:
            p = np.array([rng.uniform(8, 744), rng.uniform(8, 472)])
            if apart(p):
                break
        pts = np.vstack([pts, p])
    return pts[rng.permutation(len(pts))]


def problems(n_bodies, strays, n, seed):
    return [dict(cameras=[(K, np.eye(4))], dets=[scene(np.random.default_rng([seed, n_bodies, k]), n_bodies, strays)])
            for k in range(n)]


def parents_way(h, ps, n_bodies):
    """one rig_init_batch call per body over all problems, the claimed points filtered out on the host in between"""
    cameras, tol = ps[0]["cameras"], 3.0
    keep = [np.arange(len(p["dets"][0])) for p in ps]
    found = 0
    for b in range(n_bodies):
        lists = [[p["dets"][0][k]] for p, k in zip(ps, keep)]
        rec, match, info = h.rig_init_batch(cameras, synth.M5, lists, tol, tol, min_rows=5, min_markers=5, min_margin=0)
        for i in range(len(ps)):
            if info[i]["reason"] == 0:
                found += 1
                w = match[i][0]
                keep[i] = np.delete(keep[i], w[w != 0].astype(np.int64) - 1)
    return found


def main(path):
    h = mpe.Handle()
    tool = "python tools/rig_init_bodies_numbers.py"
    with open(path, "a") as fh:
        for n_bodies, strays in ((2, 4), (4, 8)):
            for n in (1, 1024):
                ps = problems(n_bodies, strays, n, 20261021)
                bodies = [(synth.M5, None)] * n_bodies
                dets = [p["dets"] for p in ps]
                for way in ("rig_init_bodies_batch", "rig_init_batch_per_body"):
                    for rep in range(4):  # (the first is the warm-up)
                        t0 = time.perf_counter()
                        if way == "rig_init_bodies_batch":
                            rec, match, info, owner = h.rig_init_bodies_batch(ps[0]["cameras"], bodies, dets, 3.0, 3.0)
                            found = int((info["reason"] == 0).sum())
                        else:
                            found = parents_way(h, ps, n_bodies)
                        dt = time.perf_counter() - t0
                        if rep == 0:
                            continue
                        line = dict(tool=tool, way=way, bodies=n_bodies, markers=5, strays=strays, problems=n, points=len(dets[0][0]),
                                    repetition=rep, wall_us=round(dt * 1e6, 1), bodies_found=found,
                                    submissions=1 if way == "rig_init_bodies_batch" else n_bodies)
                        fh.write(json.dumps(line) + "\n")
                        print(line)
    h.close()


if __name__ == "__main__":
    main(sys.argv[1])
