"""A numpy witness of the marker calibration (include/mpe.h, mpe_body_calibrate), written in ANOTHER formulation than the
device code on purpose.  The device code multiplies the reference's closed-form Jacobian at q by the adjoint of the
extrinsic, eliminates the view poses with a Schur complement, adds w N N^T to the singular reduced system and factors
with unpivoted LDL^T; here there is ONE dense Jacobian over all unknowns, ordered [delta of the free markers, ascending |
xi of the used views],

    q = E_c X,  X = T_f p_m,   Jm = P R_c R_f             (additive delta on p_m),
                               Jp = P R_c [I | -hat(X)]   (left twist xi on T_f),
    P = [[fx / z, 0, -fx x / z^2], [0, fy / z, -fy y / z^2]],

and the inner constraints are not a penalty but the border of a KKT system,

    [[J^T J, C], [C^T, 0]] [Delta; lambda] = [J^T e; 0],   C = [N; 0],

solved with np.linalg.solve.  N (3 n_free x 6 or 7): with c the centroid of the free markers' current positions and d_m =
p_m - c, the columns are the three translations (e_k)_m, the three rotations (e_k x d_m)_m and, when scale is held,
(d_m)_m.  The covariance is the 3 x 3 diagonal blocks of np.linalg.pinv of the dense reduced system S = A_mm - A_mv
A_vv^-1 A_vm of the last iteration, restricted to the constraints (P S P with P = I - N (N^T N)^-1 N^T: the same matrix
up to rounding while N spans null vectors of S, and the covariance of the constrained estimate when a scale the rig
observes is held; rcond 1e-10: the six or seven eigenvalues that vanish are ~1e-16 of the largest, the others >= 1e-6 of
it on the problems drawn here).  Same residual, left-multiplicative pose update
(witness_pipeline.exponential_map), stop rule (largest |component| of the step <= step_tolerance behind the update, or
max_iterations) and the same rules for which rows take part — a fixed point that starts with every marker free:

  * a view is used when its rows on free markers number >= 4 and name >= 3 distinct free markers;
  * a marker is free when it has >= 2 rows in used views; a marker that is not is held: state 2, position unchanged,
    rows dropped;
  * scale: -1 held exactly when no used view has used rows of two cameras, 0 free, 1 held;
  * marker state 1 = calibrated, 2 = held; a non-finite result hands everything back as given."""
import numpy as np

import witness_rig
from witness_pipeline import exponential_map
from witness_rig_ba import _hat_rows


def plan(n_markers, views):
    """views: row lists of (camera, marker index, uv) -> (view_used [bool], marker_state, marker_rows, two_cameras)"""
    free = set(range(n_markers))
    while True:
        on_free = [[r for r in rows if r[1] in free] for rows in views]
        used = [len(rows) >= 4 and len({r[1] for r in rows}) >= 3 for rows in on_free]
        count = {m: sum(1 for rows, u in zip(on_free, used) if u for r in rows if r[1] == m) for m in free}
        keep = {m for m in free if count[m] >= 2}
        if keep == free:
            break
        free = keep
    state = [1 if m in free else 2 for m in range(n_markers)]
    rows_of = [count.get(m, 0) for m in range(n_markers)]
    two = any(u and len({r[0] for r in rows}) >= 2 for rows, u in zip(on_free, used))
    return used, state, rows_of, two


def gauge(p_free, scale_held):
    """p_free (n, 3) -> N (3 n, 6 or 7)"""
    d = p_free - p_free.mean(axis=0)
    cols = [np.tile(np.eye(3)[k], len(d)) for k in range(3)]
    cols += [np.cross(np.eye(3)[k], d).reshape(-1) for k in range(3)]
    if scale_held:
        cols.append(d.reshape(-1))
    return np.stack(cols, 1)


def body_calibrate(cameras, views, markers, T_views, scale=-1, max_iterations=50, step_tolerance=1e-10):
    """cameras: list of (K 3x3, E 4x4 camera <- rig); views: list of row lists, a row = (camera index, marker index,
    pixel uv); markers: (n, 3) START positions; T_views: (n_views, 4, 4) start poses, rig <- marker frame.
    -> dict(markers (n, 3), T_views, cov (n, 3, 3), view_used, report dict, ok)."""
    p0 = np.array(markers, float).reshape(-1, 3)
    n_mk = len(p0)
    used, state, rows_of, two = plan(n_mk, views)
    T0 = np.array(T_views, float).reshape(-1, 4, 4)
    free = [m for m in range(n_mk) if state[m] == 1]
    held = (not two) if scale < 0 else bool(scale)
    out = dict(markers=p0.copy(), T_views=T0.copy(), cov=np.zeros((n_mk, 3, 3)), view_used=np.array(used, bool), ok=False)
    report = dict(status=1, iterations=0, views_used=int(sum(used)), rows_used=int(sum(rows_of)), markers_free=len(free),
                  scale_held=int(held), rms_before=0.0, rms_after=0.0, last_step=0.0, marker_state=state, marker_rows=rows_of)
    out["report"] = report
    uv_idx = [f for f in range(len(views)) if used[f]]
    if len(free) < 3 or not uv_idx:
        return out
    nm = 3 * len(free)
    col_m = {m: 3 * i for i, m in enumerate(free)}
    col_v = {f: nm + 6 * i for i, f in enumerate(uv_idx)}
    n_unk = nm + 6 * len(uv_idx)
    rows = [(f, r) for f in uv_idx for r in views[f] if state[r[1]] == 1]
    rc = np.array([r[0] for _, r in rows])
    rm = np.array([r[1] for _, r in rows])
    rf = np.array([f for f, _ in rows])
    uv = np.array([r[2] for _, r in rows], float)
    Kc = np.array([np.asarray(K, float).reshape(3, 3) for K, _ in cameras])
    E = np.array([np.asarray(Ec, float).reshape(4, 4) for _, Ec in cameras])
    fx, fy, cx, cy = Kc[rc, 0, 0], Kc[rc, 1, 1], Kc[rc, 0, 2], Kc[rc, 1, 2]
    n = len(rc)
    cm = np.array([col_m[m] for m in rm])
    cp = np.array([col_v[f] for f in rf])
    p, T = p0.copy(), T0.copy()

    def linearise():
        X = np.einsum("nij,nj->ni", T[rf, :3, :3], p[rm]) + T[rf, :3, 3]
        q = np.einsum("nij,nj->ni", E[rc, :3, :3], X) + E[rc, :3, 3]
        x, y, z = q.T
        e = uv - np.stack([fx * x / z + cx, fy * y / z + cy], 1)
        P = np.zeros((n, 2, 3))
        P[:, 0, 0], P[:, 0, 2] = fx / z, -fx * x / z ** 2
        P[:, 1, 1], P[:, 1, 2] = fy / z, -fy * y / z ** 2
        PR = np.einsum("nij,njk->nik", P, E[rc, :3, :3])
        Jm = np.einsum("nij,njk->nik", PR, T[rf, :3, :3])
        Jp = np.einsum("nij,njk->nik", PR, np.concatenate([np.tile(np.eye(3), (n, 1, 1)), -_hat_rows(X)], 2))
        return e, Jm, Jp

    A = np.eye(n_unk)
    sse_before = step = 0.0
    iters = 0
    with np.errstate(all="ignore"):
        for it in range(max_iterations):
            e, Jm, Jp = linearise()
            if it == 0:
                sse_before = float((e ** 2).sum())
            J = np.zeros((2 * n, n_unk))
            for k in range(n):
                J[2 * k:2 * k + 2, cm[k]:cm[k] + 3] = Jm[k]
                J[2 * k:2 * k + 2, cp[k]:cp[k] + 6] = Jp[k]
            A = J.T @ J
            b = J.T @ e.reshape(-1)
            N = gauge(p[free], held)
            k_con = N.shape[1]
            KKT = np.zeros((n_unk + k_con, n_unk + k_con))
            KKT[:n_unk, :n_unk] = A
            KKT[:nm, n_unk:] = N
            KKT[n_unk:, :nm] = N.T
            try:
                d = np.linalg.solve(KKT, np.concatenate([b, np.zeros(k_con)]))[:n_unk]
            except np.linalg.LinAlgError:
                d = np.full(n_unk, np.nan)
            p[free] += d[:nm].reshape(-1, 3)
            for f in uv_idx:
                T[f] = exponential_map(d[col_v[f]:col_v[f] + 6]) @ T[f]
            iters = it + 1
            step = float(np.abs(d).max())
            if not step > step_tolerance:
                break
        try:
            S = A[:nm, :nm] - A[:nm, nm:] @ np.linalg.solve(A[nm:, nm:], A[nm:, :nm])
            Pn = np.eye(nm) - N @ np.linalg.solve(N.T @ N, N.T)
            S = Pn @ ((S + S.T) / 2) @ Pn
            Sp = np.linalg.pinv((S + S.T) / 2, rcond=1e-10, hermitian=True)
        except np.linalg.LinAlgError:
            Sp = np.full((nm, nm), np.nan)
        e, _, _ = linearise()
    sse_after = float((e ** 2).sum())
    cov = np.zeros((n_mk, 3, 3))
    for m in free:
        cov[m] = Sp[col_m[m]:col_m[m] + 3, col_m[m]:col_m[m] + 3]
    report.update(iterations=iters, rms_before=float(np.sqrt(sse_before / (2 * n))), rms_after=float(np.sqrt(sse_after / (2 * n))),
                  last_step=step)
    if not (np.isfinite(p).all() and np.isfinite(T).all() and np.isfinite(cov).all() and np.isfinite([sse_before, sse_after]).all()):
        return out
    report["status"] = 0
    out.update(markers=p, T_views=T, cov=cov, ok=True)
    return out


def align(shape, target, with_scale):
    """shape (n, 3) moved rigidly (and scaled, with_scale) onto target in the least-squares sense (Kabsch / Umeyama)."""
    a, b = shape - shape.mean(0), target - target.mean(0)
    U, s, Vt = np.linalg.svd(a.T @ b)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = (U @ D @ Vt).T
    k = (s * D.diagonal()).sum() / (a ** 2).sum() if with_scale else 1.0
    return k * a @ R.T + target.mean(0)


def shape_error(shape, target, with_scale):
    """the largest distance of a marker of `shape`, aligned onto `target`, from its counterpart"""
    return float(np.linalg.norm(align(np.asarray(shape, float), np.asarray(target, float), with_scale) - target, axis=1).max())


# ---- random calibration problems (CPU tier and GPU tier draw from the same generator) ------------------------------

def random_body_calibration(rng, n_cam, n_views, n_markers=5, p_missing=0.2, noise=0.1, ruler_error=0.004, exact=False):
    """A body of n_markers LEDs (+-0.25 m) in front of n_cam cameras (witness_rig.random_cameras; one camera: the identity)
    in n_views views up to 1.2 rad apart, 1.2 - 2.2 m away: every (camera, marker) row of a view is missing with
    probability p_missing; pixels with `noise` px of Gaussian noise, rounded through float32 (exact: neither).  The start
    markers are the true ones plus ruler_error m of Gaussian error (per marker, rms), the start poses 0.05 rad / 0.01 m
    off.  -> dict(cameras, views, markers (start), markers_true, T_start, T_true)."""
    truth = rng.uniform(-0.25, 0.25, (n_markers, 3))
    cams = witness_rig.random_cameras(rng, n_cam, identity_first=n_cam == 1)
    views, T_true = [], []
    for f in range(n_views):
        Tt = witness_rig._rigid(rng, rng.uniform(0, 1.2), [rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(1.2, 2.2)])
        rows = []
        for c, (K, E) in enumerate(cams):
            for m in range(n_markers):
                if rng.random() < p_missing:
                    continue
                q = (E @ Tt @ np.append(truth[m], 1.0))[:3]
                uv = np.array([K[0, 0] * q[0] / q[2] + K[0, 2], K[1, 1] * q[1] / q[2] + K[1, 2]])
                if not exact:
                    uv = (uv + rng.normal(0, noise, 2)).astype(np.float32).astype(np.float64)
                rows.append((c, m, uv))
        views.append(rows)
        T_true.append(Tt)
    start = truth + rng.normal(size=(n_markers, 3)) * ruler_error / np.sqrt(3)
    T_start = np.array([witness_rig._rigid(rng, 0.05, rng.normal(size=3) * 0.01 / np.sqrt(3)) @ T for T in T_true])
    return dict(cameras=cams, views=views, markers=start, markers_true=truth, T_start=T_start, T_true=np.array(T_true))


def check_against_witness(got, prob, what=None, **kw):
    """witness_rig_ba.check_against_witness's criteria for this refinement: marker positions and view poses within 1e-9,
    covariance allclose(rtol=1e-5, atol=1e-12), iteration counts within +-1; states, counts and flags equal.
    got: dict(markers, T_views, cov, view_used, report) as Handle.body_calibrate returns it.  -> the witness's result."""
    w = body_calibrate(prob["cameras"], prob["views"], prob["markers"], prob["T_start"], **kw)
    rg, rw = got["report"], w["report"]
    n_mk = len(rw["marker_state"])
    assert rg["status"] == rw["status"], (what, rg["status"], rw["status"])
    assert list(rg["marker_state"][:n_mk]) == rw["marker_state"], what
    assert list(rg["marker_rows"][:n_mk]) == rw["marker_rows"], what
    assert rg["views_used"] == rw["views_used"] and rg["rows_used"] == rw["rows_used"], what
    assert rg["markers_free"] == rw["markers_free"] and rg["scale_held"] == rw["scale_held"], what
    assert np.array_equal(np.asarray(got["view_used"], bool), w["view_used"]), what
    assert abs(rg["iterations"] - rw["iterations"]) <= 1, (what, rg["iterations"], rw["iterations"])
    dP = np.abs(np.asarray(got["markers"]).reshape(-1, 3) - w["markers"]).max()
    dT = np.abs(np.asarray(got["T_views"]).reshape(-1, 4, 4) - w["T_views"]).max() if len(w["T_views"]) else 0.0
    assert dP <= 1e-9 and dT <= 1e-9, (what, dP, dT)
    assert np.allclose(np.asarray(got["cov"]).reshape(-1, 3, 3), w["cov"], rtol=1e-5, atol=1e-12), what
    if rw["status"] == 0:
        # (as witness_rig_ba: the same start values, rounding only; final values within 1e-9 move a pixel by < 5e-6 px)
        assert np.isclose(rg["rms_before"], rw["rms_before"], rtol=1e-9, atol=0), what
        assert abs(rg["rms_after"] - rw["rms_after"]) <= 1e-5, what
    return w
