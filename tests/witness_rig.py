"""A numpy witness of the rig refinement (include/mpe.h, mpe_rig_optimise_pose_batch), written in ANOTHER formulation
than the device code on purpose: the device code multiplies the reference's closed-form Jacobian at q by the adjoint of
the camera's extrinsic; here the chain rule is taken the other way round,

    q = R_c X + t_c,  X = T p,   d q / d xi = R_c [I | -hat(X)]   (left twist xi = (upsilon, omega) on T),
    J = P R_c [I | -hat(X)],     P = [[fx / z, 0, -fx x / z^2], [0, fy / z, -fy y / z^2]]  (2 x 3 projection Jacobian),

the normal equations are solved with np.linalg.solve (LU with pivoting, not LDL^T) and the update is
witness_pipeline.exponential_map.  Same residual, twist order, left-multiplicative update, stop rule (max|dT| <= 1e-13
behind the update, 500 iterations at most) and covariance (inverse of the last iteration's A)."""
import numpy as np

from rpg_monocular_pose_estimator_amd import synth
from witness_pipeline import exponential_map


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rig_optimise_pose(cameras, rows, T_init):
    """cameras: list of (K 3x3, E 4x4 camera <- rig); rows: list of (camera index, marker xyz, pixel uv) in summation
    order; T_init 4x4 (rig <- marker frame) -> (T 4x4, cov 6x6, iterations, status)."""
    T = np.array(T_init, float).reshape(4, 4).copy()
    T[3] = [0, 0, 0, 1]
    if len(rows) < 3:
        return T, np.zeros((6, 6)), 0, 1
    A = np.zeros((6, 6))
    iters = 0
    for it in range(500):
        A = np.zeros((6, 6))
        b = np.zeros(6)
        for c, p, uv in rows:
            K, E = cameras[c]
            K, E = np.asarray(K, float).reshape(3, 3), np.asarray(E, float).reshape(4, 4)
            fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
            R = E[:3, :3]
            X = T[:3, :3] @ np.asarray(p, float) + T[:3, 3]
            x, y, z = R @ X + E[:3, 3]
            e = np.asarray(uv, float) - np.array([fx * x / z + cx, fy * y / z + cy])
            P = np.array([[fx / z, 0.0, -fx * x / z ** 2], [0.0, fy / z, -fy * y / z ** 2]])
            J = P @ R @ np.hstack([np.eye(3), -hat(X)])
            A += J.T @ J
            b += J.T @ e
        with np.errstate(all="ignore"):
            try:
                dT = np.linalg.solve(A, b)
            except np.linalg.LinAlgError:
                dT = np.full(6, np.nan)
        T = exponential_map(dT) @ T
        iters = it + 1
        if not np.abs(dT).max() > 1e-13:  # (a NaN step ends the loop too, as the reference's norm_max does)
            break
    with np.errstate(all="ignore"):
        try:
            cov = np.linalg.inv(A)
        except np.linalg.LinAlgError:
            cov = np.full((6, 6), np.nan)
    return T, cov, iters, 0 if np.isfinite(T).all() else 1


# ---- random rigs for the tests (CPU tier and GPU tier draw from the same generators) -------------------------------

def _rigid(rng, angle, shift):
    ax = rng.normal(size=3)
    T = np.eye(4)
    T[:3, :3] = synth.rodrigues(ax / np.linalg.norm(ax), angle)
    T[:3, 3] = shift
    return T


def random_cameras(rng, n_cam, identity_first=False):
    """n_cam cameras (K, E): focal lengths 400 - 460, extrinsics up to 0.5 rad and 0.3 m."""
    cams = []
    for c in range(n_cam):
        K = np.array([[rng.uniform(400, 460), 0, rng.uniform(360, 390)], [0, rng.uniform(400, 460), rng.uniform(230, 250)],
                      [0, 0, 1]])
        E = np.eye(4) if (identity_first and c == 0) else _rigid(rng, rng.uniform(0, 0.5), rng.uniform(-0.3, 0.3, 3))
        cams.append((K, E))
    return cams


def random_problem(rng, cameras, seen, markers):
    """One problem over `cameras`: camera c sees seen[c] of the markers (a random subset, ascending), pixels with 0.1 px
    noise rounded through float32, the start 0.05 rad / 0.01 m off the true pose.  -> (rows, T_init)."""
    T_true = _rigid(rng, rng.uniform(0, 0.6), [rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(1.2, 2.2)])
    rows = []
    for c, (K, E) in enumerate(cameras):
        for m in sorted(rng.permutation(len(markers))[:seen[c]]):
            q = (E @ T_true @ np.append(markers[m], 1.0))[:3]
            uv = np.array([K[0, 0] * q[0] / q[2] + K[0, 2], K[1, 1] * q[1] / q[2] + K[1, 2]]) + rng.normal(0, 0.1, 2)
            rows.append((c, markers[m].copy(), uv.astype(np.float32).astype(np.float64)))
    T0 = _rigid(rng, 0.05, rng.normal(size=3) * 0.01 / np.sqrt(3)) @ T_true
    return rows, T0


def random_rig(rng, n_cam=None, seen=None, n_markers=5):
    """A rig and one problem: 1 - 8 cameras (or n_cam), camera 0 sees >= 4 of the 5 markers and the others 1 - 5 (or
    `seen` per camera).  -> (cameras, rows, T_init)."""
    n_cam = int(rng.integers(1, 9)) if n_cam is None else n_cam
    markers = rng.uniform(-0.25, 0.25, (n_markers, 3))
    cameras = random_cameras(rng, n_cam)
    if seen is None:
        seen = [int(rng.integers(4, 6)) if c == 0 else int(rng.integers(1, 6)) for c in range(n_cam)]
    rows, T0 = random_problem(rng, cameras, seen, markers)
    return cameras, rows, T0


def check_against_witness(rec, cameras, rows, T0, what=None):
    """The criteria the project applies to this refinement against its oracle (tests/test_gpu_parity.py:801-804): pose
    within 1e-9, covariance allclose(rtol=1e-5, atol=1e-12), iteration counts within +-1.  -> the witness's count."""
    T_w, cov_w, it_w, st_w = rig_optimise_pose(cameras, rows, T0)
    assert rec["status"] == st_w, what
    assert abs(int(rec["gn_iterations"]) - it_w) <= 1, (what, int(rec["gn_iterations"]), it_w)
    assert np.abs(rec["T"].reshape(4, 4) - T_w).max() <= 1e-9, (what, np.abs(rec["T"].reshape(4, 4) - T_w).max())
    assert np.allclose(rec["cov"].reshape(6, 6), cov_w, rtol=1e-5, atol=1e-12), what
    return it_w
