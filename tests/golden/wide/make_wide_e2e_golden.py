#!/usr/bin/env python
"""Generates tests/golden/wide/wide_e2e.npz — the oracle's estimateBodyPose records of the 8 frames of
tests/test_wide_frames.e2e_frames (two of them wide: 70 and 130 spots against 5 markers, 3.3 M and 21 M hypotheses —
more than a minute of one core, too long for a test; the oracle initialises the 70-spot one).  The frames are not stored: a SHA-1 per frame detects drift.

    python tests/golden/wide/make_wide_e2e_golden.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

import oracle  # noqa: E402
from rpg_monocular_pose_estimator_amd import synth  # noqa: E402
from test_wide_frames import e2e_frames, E2E_TOL  # noqa: E402

frames, K, D = e2e_frames()
rec = oracle.estimate_batch(frames, synth.M5, K, D, oracle.make_params(back_projection_pixel_tolerance=E2E_TOL), n_threads=8)
np.savez_compressed(os.path.join(HERE, "wide_e2e.npz"), sha1=np.array([hashlib.sha1(f.tobytes()).hexdigest() for f in frames]),
                    tol=E2E_TOL, status=rec["status"], n_det=rec["n_det"], n_corr=rec["n_corr"], T=rec["T"], cov=rec["cov"])
print("status", rec["status"].tolist(), "n_det", rec["n_det"].tolist(), "n_corr", rec["n_corr"].tolist())
