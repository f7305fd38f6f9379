"""A numpy witness of the rig calibration (include/mpe.h, mpe_rig_calibrate), written in ANOTHER formulation than the
device code on purpose.  The device code multiplies the reference's closed-form Jacobian at q by the adjoint of the
extrinsic, eliminates the view poses with a Schur complement and factors with unpivoted LDL^T; here there is ONE dense
Jacobian over all unknowns, ordered [eta of the free cameras, ascending | xi of the used views],

    q = E_c X,  X = T_f p,   Je = P [I | -hat(q)]      (left twist eta on E_c),
                             Jp = P R_c [I | -hat(X)]  (left twist xi on T_f),
    P = [[fx / z, 0, -fx x / z^2], [0, fy / z, -fy y / z^2]],

np.linalg.solve on the full normal equations, the covariance as the diagonal 6 x 6 blocks of their full inverse, and the
update is witness_pipeline.exponential_map.  Same residual, twist order, left-multiplicative updates, gauge (the reference
camera keeps its extrinsic), stop rule (largest |component| of the step <= step_tolerance behind the update, or
max_iterations) and the same rules for which rows take part:

  * a view is a candidate with >= 3 rows of >= 2 distinct cameras; cameras are linked by candidate views;
  * a camera outside the reference camera's connected component (a camera without rows among them) is held: state 2,
    extrinsic unchanged, rows dropped; a view is used when it is a candidate of cameras in that component;
  * camera state 0 = reference, 1 = calibrated, 2 = held; a non-finite result hands everything back as given."""
import numpy as np

import witness_rig
from witness_pipeline import exponential_map


def plan(n_cam, views, ref):
    """-> (view_used [bool], camera_state [int], camera_rows [int])"""
    cand = [len(rows) >= 3 and len({r[0] for r in rows}) >= 2 for rows in views]
    linked, grown = {ref}, True
    while grown:                                         # (a flood fill: no union-find here)
        grown = False
        for rows, ok in zip(views, cand):
            cams = {r[0] for r in rows}
            if ok and cams & linked and not cams <= linked:
                linked |= cams
                grown = True
    used = [ok and {r[0] for r in rows} <= linked for rows, ok in zip(views, cand)]
    rows_of = [0] * n_cam
    for rows, u in zip(views, used):
        if u:
            for r in rows:
                rows_of[r[0]] += 1
    state = [0 if c == ref else (1 if rows_of[c] > 0 and rows_of[ref] > 0 else 2) for c in range(n_cam)]
    return used, state, rows_of


def _hat_rows(v):
    """(n, 3) -> (n, 3, 3) of hat(v)"""
    H = np.zeros((len(v), 3, 3))
    H[:, 0, 1], H[:, 0, 2] = -v[:, 2], v[:, 1]
    H[:, 1, 0], H[:, 1, 2] = v[:, 2], -v[:, 0]
    H[:, 2, 0], H[:, 2, 1] = -v[:, 1], v[:, 0]
    return H


def rig_calibrate(cameras, views, T_views, reference_camera=0, max_iterations=50, step_tolerance=1e-10):
    """cameras: list of (K 3x3, E 4x4 camera <- rig, the START extrinsics); views: list of row lists, a row = (camera
    index, marker xyz, pixel uv); T_views: (n, 4, 4) start poses, rig <- marker frame.
    -> dict(T_cam_rig (n_cam, 4, 4), T_views, cov (n_cam, 6, 6), view_used, report dict, ok)."""
    n_cam, ref = len(cameras), reference_camera
    used, state, rows_of = plan(n_cam, views, ref)
    E0 = np.array([np.asarray(E, float).reshape(4, 4) for _, E in cameras])
    T0 = np.array(T_views, float).reshape(-1, 4, 4)
    out = dict(T_cam_rig=E0.copy(), T_views=T0.copy(), cov=np.zeros((n_cam, 6, 6)), view_used=np.array(used, bool), ok=False)
    report = dict(status=1, iterations=0, views_used=int(sum(used)), rows_used=int(sum(rows_of)), rms_before=0.0,
                  rms_after=0.0, last_step=0.0, camera_state=state, camera_rows=rows_of)
    out["report"] = report
    free = [c for c in range(n_cam) if state[c] == 1]
    uv_idx = [f for f in range(len(views)) if used[f]]
    if not free or not uv_idx:
        return out
    col_cam = {c: 6 * i for i, c in enumerate(free)}
    col_view = {f: 6 * len(free) + 6 * i for i, f in enumerate(uv_idx)}
    n_unk = 6 * (len(free) + len(uv_idx))
    rc = np.array([r[0] for f in uv_idx for r in views[f]])
    rf = np.array([f for f in uv_idx for r in views[f]])
    p = np.array([r[1] for f in uv_idx for r in views[f]], float)
    uv = np.array([r[2] for f in uv_idx for r in views[f]], float)
    Kc = np.array([np.asarray(K, float).reshape(3, 3) for K, _ in cameras])
    fx, fy, cx, cy = Kc[rc, 0, 0], Kc[rc, 1, 1], Kc[rc, 0, 2], Kc[rc, 1, 2]
    n = len(rc)
    ce = np.array([col_cam.get(c, -1) for c in rc])
    cp = np.array([col_view[f] for f in rf])
    E, T = E0.copy(), T0.copy()

    def linearise():
        X = np.einsum("nij,nj->ni", T[rf, :3, :3], p) + T[rf, :3, 3]
        q = np.einsum("nij,nj->ni", E[rc, :3, :3], X) + E[rc, :3, 3]
        x, y, z = q.T
        e = uv - np.stack([fx * x / z + cx, fy * y / z + cy], 1)
        P = np.zeros((n, 2, 3))
        P[:, 0, 0], P[:, 0, 2] = fx / z, -fx * x / z ** 2
        P[:, 1, 1], P[:, 1, 2] = fy / z, -fy * y / z ** 2
        Je = np.einsum("nij,njk->nik", P, np.concatenate([np.tile(np.eye(3), (n, 1, 1)), -_hat_rows(q)], 2))
        Jp = np.einsum("nij,njk,nkl->nil", P, E[rc, :3, :3], np.concatenate([np.tile(np.eye(3), (n, 1, 1)), -_hat_rows(X)], 2))
        return e, Je, Jp

    A = np.eye(n_unk)
    sse_before = step = 0.0
    iters = 0
    with np.errstate(all="ignore"):
        for it in range(max_iterations):
            e, Je, Jp = linearise()
            if it == 0:
                sse_before = float((e ** 2).sum())
            J = np.zeros((2 * n, n_unk))
            for k in range(n):
                if ce[k] >= 0:
                    J[2 * k:2 * k + 2, ce[k]:ce[k] + 6] = Je[k]
                J[2 * k:2 * k + 2, cp[k]:cp[k] + 6] = Jp[k]
            A = J.T @ J
            b = J.T @ e.reshape(-1)
            try:
                d = np.linalg.solve(A, b)
            except np.linalg.LinAlgError:
                d = np.full(n_unk, np.nan)
            for c in free:
                E[c] = exponential_map(d[col_cam[c]:col_cam[c] + 6]) @ E[c]
            for f in uv_idx:
                T[f] = exponential_map(d[col_view[f]:col_view[f] + 6]) @ T[f]
            iters = it + 1
            step = float(np.abs(d).max())
            if not step > step_tolerance:
                break
        try:
            Ainv = np.linalg.inv(A)
        except np.linalg.LinAlgError:
            Ainv = np.full((n_unk, n_unk), np.nan)
        e, _, _ = linearise()
    sse_after = float((e ** 2).sum())
    cov = np.zeros((n_cam, 6, 6))
    for c in free:
        cov[c] = Ainv[col_cam[c]:col_cam[c] + 6, col_cam[c]:col_cam[c] + 6]
    report.update(iterations=iters, rms_before=float(np.sqrt(sse_before / (2 * n))), rms_after=float(np.sqrt(sse_after / (2 * n))),
                  last_step=step)
    if not (np.isfinite(E).all() and np.isfinite(T).all() and np.isfinite(cov).all() and np.isfinite([sse_before, sse_after]).all()):
        return out
    report["status"] = 0
    out.update(T_cam_rig=E, T_views=T, cov=cov, ok=True)
    return out


# ---- random calibration problems (CPU tier and GPU tier draw from the same generator) ------------------------------

def random_calibration(rng, n_cam, n_views, n_markers=5, seen=(3, 5), p_missing=0.3, noise=0.1, reference_camera=0,
                       perturb=True):
    """A rig of n_cam cameras (witness_rig.random_cameras) and n_views views of one body: every camera is missing from a
    view with probability p_missing, else it sees seen[0] .. seen[1] of the markers (a random subset, ascending); pixels
    with `noise` px of Gaussian noise, rounded through float32.  Start extrinsics 0.03 rad / 0.01 m off the truth (the
    reference camera's is the truth: the gauge), start poses 0.05 rad / 0.01 m off.
    -> dict(cameras (start), E_true (n_cam, 4, 4), views, T_start, T_true)."""
    markers = rng.uniform(-0.25, 0.25, (n_markers, 3))
    cams = witness_rig.random_cameras(rng, n_cam)
    E_true = np.array([E for _, E in cams])
    views, T_true = [], []
    for f in range(n_views):
        Tt = witness_rig._rigid(rng, rng.uniform(0, 0.6), [rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(1.2, 2.2)])
        rows = []
        for c, (K, E) in enumerate(cams):
            if rng.random() < p_missing:
                continue
            k = int(rng.integers(seen[0], seen[1] + 1))
            for m in sorted(rng.permutation(n_markers)[:k]):
                q = (E @ Tt @ np.append(markers[m], 1.0))[:3]
                uv = np.array([K[0, 0] * q[0] / q[2] + K[0, 2], K[1, 1] * q[1] / q[2] + K[1, 2]]) + rng.normal(0, noise, 2)
                rows.append((c, markers[m].copy(), uv.astype(np.float32).astype(np.float64)))
        views.append(rows)
        T_true.append(Tt)
    start = []
    for c, (K, E) in enumerate(cams):
        off = np.eye(4) if (c == reference_camera or not perturb) else witness_rig._rigid(rng, 0.03, rng.normal(size=3) * 0.01 / np.sqrt(3))
        start.append((K, off @ E))
    T_start = np.array([(witness_rig._rigid(rng, 0.05, rng.normal(size=3) * 0.01 / np.sqrt(3)) if perturb else np.eye(4)) @ T
                        for T in T_true])
    return dict(cameras=start, E_true=E_true, views=views, T_start=T_start, T_true=np.array(T_true))


def check_against_witness(got, prob, what=None, **kw):
    """The criteria of witness_rig.check_against_witness for this refinement: extrinsics and view poses within 1e-9,
    covariance allclose(rtol=1e-5, atol=1e-12), iteration counts within +-1; states, counts and flags equal.
    got: dict(T_cam_rig, T_views, cov, view_used, report) as Handle.rig_calibrate returns it.  -> the witness's result."""
    w = rig_calibrate(prob["cameras"], prob["views"], prob["T_start"], **kw)
    rg, rw = got["report"], w["report"]
    assert rg["status"] == rw["status"], (what, rg["status"], rw["status"])
    assert list(rg["camera_state"][:len(rw["camera_state"])]) == rw["camera_state"], what
    assert list(rg["camera_rows"][:len(rw["camera_rows"])]) == rw["camera_rows"], what
    assert rg["views_used"] == rw["views_used"] and rg["rows_used"] == rw["rows_used"], what
    assert np.array_equal(np.asarray(got["view_used"], bool), w["view_used"]), what
    assert abs(rg["iterations"] - rw["iterations"]) <= 1, (what, rg["iterations"], rw["iterations"])
    dE = np.abs(np.asarray(got["T_cam_rig"]).reshape(-1, 4, 4) - w["T_cam_rig"]).max()
    dT = np.abs(np.asarray(got["T_views"]).reshape(-1, 4, 4) - w["T_views"]).max() if len(w["T_views"]) else 0.0
    assert dE <= 1e-9 and dT <= 1e-9, (what, dE, dT)
    assert np.allclose(np.asarray(got["cov"]).reshape(-1, 6, 6), w["cov"], rtol=1e-5, atol=1e-12), what
    if rw["status"] == 0:
        # the same start values: rounding only.  The final values agree to 1e-9 per entry of E and T, a pixel moves by
        # less than f / z * (1 + |X|) * (a handful of entries) < 5e3 px per unit of them: 5e-6 px
        assert np.isclose(rg["rms_before"], rw["rms_before"], rtol=1e-9, atol=0), what
        assert abs(rg["rms_after"] - rw["rms_after"]) <= 1e-5, what
    return w
