#!/usr/bin/env python
"""Generates tests/golden/wide/wide_256x4.npz — one detection set of 256 points against 4 markers, voted and solved by
the CPU oracle (initialise + optimisePose): 66 M hypotheses, about a minute and a half of one core per pass, too long
for a test.  The set is a demo scene (4 LEDs of a random pose + 252 distractor spots >= 12 px apart, drawn by
synth.sample_scene); a detection that a winning correspondence names is then moved to the LAST place of the set and the
oracle run again, so that the expected rows hold the 1-based detection index 256 — an index a byte cannot hold.

    python tests/golden/wide/make_wide_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))

import oracle  # noqa: E402
from rpg_monocular_pose_estimator_amd import synth  # noqa: E402

N_DET, SEED, TOL = 256, 9256, 5.0


def main():
    rows, cols = 480, 752
    K, D = synth.camera_for(rows, cols)
    markers = synth.M5[:4]
    rng = np.random.default_rng(SEED)
    _, det = synth.sample_scene(rng, markers, K, D, rows, cols, n_distractors=N_DET - len(markers))
    assert det.shape == (N_DET, 2)
    det = det[rng.permutation(N_DET)]
    P = oracle.make_params(back_projection_pixel_tolerance=TOL)
    for attempt in range(4):
        r = oracle.solve_bruteforce(det, markers, K, P)
        print("pass", attempt, "status", r["status"], "rows", r["corr"].tolist(), flush=True)
        assert r["n_corr"] >= 1, "no correspondence row to place"
        if (r["corr"][:, 1] == N_DET).any():
            break
        d = int(r["corr"][0, 1]) - 1          # the detection of the strongest row goes to the last place
        det[[d, N_DET - 1]] = det[[N_DET - 1, d]]
    else:
        raise SystemExit("no pass named detection %d" % N_DET)
    np.savez_compressed(os.path.join(HERE, "wide_256x4.npz"), det=det, markers=markers, K=K, tol=TOL, seed=SEED,
                        hist=r["hist"].astype(np.uint32), corr=r["corr"].astype(np.uint32), n_corr=np.int32(r["n_corr"]),
                        status=np.int32(r["status"]), n_det=np.int32(r["n_det"]), T=r["T"], cov=r["cov"],
                        gn_iterations=np.int32(r["gn_iterations"]))
    print("wide_256x4: status", r["status"], "n_corr", r["n_corr"], "max votes", int(r["hist"].max()))


if __name__ == "__main__":
    main()
