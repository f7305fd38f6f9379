"""CPU tier of mpe_rig_init_bodies_batch (several bodies in one frame): the peel step (csrc/mpe_rig_peel.h) compiled for the
host around the host form of the rig initialiser's four steps (tests/host/rig_peel_host.cpp, behind the cut-outs
tests/test_rig_init_host.py uses) and compared with a numpy witness written as a loop around the rig initialiser's
witness (tests/witness_rig_bodies.py): EQUAL owner map, reasons, winners, best_rows, runner_rows and match words, the
records by witness_rig_init.check_against_witness' criteria.  Problems in which the witness meets a knife edge are
re-drawn; at most 1 in 10 may be.  The witness's answers are recorded in tests/golden/rig_bodies_witness.json for the GPU
tier; they must be this run's.  The entry against itself (one body = the single-body run, a round = the single-body run
over the host-filtered lists, the block count does not show — also over the full range of 1 - 4 bodies with M8 in view,
which the numpy witness cannot afford), the same source as a stand-alone program plain and under
AddressSanitizer + UndefinedBehaviorSanitizer, the new declarations of include/mpe.h (valid C99, exported, ctypes sizes,
the refusals that need no device), and the measurement behind INTEGRATION.md's table."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rpg_monocular_pose_estimator_amd as mpe
from rpg_monocular_pose_estimator_amd import synth
import test_rig_init_host as TI
import witness_rig_bodies as WB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "rig_peel_host.cpp")


def build_host(d):
    so = os.path.join(d, "librig_peel_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", *TI.extract(d), SRC, "-o", so])
    lib = C.CDLL(so)
    lib.host_rig_bodies.restype = None
    lib.host_rig_single.restype = None
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("rig_peel_host"))


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    """the single-body host build of tests/test_rig_init_host.py"""
    return TI.build_host(tmp_path_factory.mktemp("rig_init_host_for_bodies"))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _options(problem):
    opts = (mpe.MpeRigInitOptions * len(problem["bodies"]))()
    for b in range(len(problem["bodies"])):
        for k, v in WB.body_options(problem, b).items():
            setattr(opts[b], k, int(v))
    return opts


def host_bodies(host, problem, blocks=0):
    """-> (records (n_bodies), match (n_bodies, n_cam, MAX_MARKERS), info (n_bodies), owner per camera) of one problem through
    the host build"""
    cams = mpe.binding.pack_rig_cameras(problem["cameras"])
    n_cam, n_b = len(problem["cameras"]), len(problem["bodies"])
    mk = np.ascontiguousarray(np.concatenate([np.asarray(M, float).reshape(-1, 3) for M, _ in problem["bodies"]]))
    n_mk = np.array([len(M) for M, _ in problem["bodies"]], np.int32)
    lists = [np.ascontiguousarray(d, float).reshape(-1, 2) for d in problem["dets"]]
    begin = np.zeros(n_cam + 1, np.int32)
    begin[1:] = np.cumsum([len(d) for d in lists])
    xy = np.ascontiguousarray(np.concatenate(lists), float)
    cl = None if problem.get("claimed") is None else np.ascontiguousarray(np.concatenate(
        [np.asarray(f).reshape(-1) != 0 for f in problem["claimed"]]), np.uint8)
    fi = None if problem.get("find") is None else np.ascontiguousarray(np.asarray(problem["find"]) != 0, np.uint8)
    tv, ta = np.ascontiguousarray(problem["tol_vote"], float), np.ascontiguousarray(problem["tol_accept"], float)
    rec = np.zeros(n_b, mpe.RESULT_DTYPE)
    match = np.full((n_b, n_cam, mpe.MAX_MARKERS), 0xFFFFFFFF, np.uint32)
    info = np.zeros(n_b, mpe.RIG_INIT_INFO_DTYPE)
    owner = np.full(max(1, len(xy)), 99, np.int8)
    host.host_rig_bodies(cams, n_cam, _ptr(mk), _ptr(n_mk), _options(problem), n_b, _ptr(begin), _ptr(xy), _ptr(cl), _ptr(fi),
                         _ptr(tv), _ptr(ta), int(blocks), _ptr(rec), _ptr(match), _ptr(info), _ptr(owner))
    return rec, match, info, [owner[begin[c]:begin[c + 1]].copy() for c in range(n_cam)]


def host_single(host, cameras, markers, lists, tol_v, tol_a, options):
    """one body over given lists through the same build (exact block count)"""
    cams = mpe.binding.pack_rig_cameras(cameras)
    mk = np.ascontiguousarray(markers, float).reshape(-1, 3)
    lists = [np.ascontiguousarray(d, float).reshape(-1, 2) for d in lists]
    begin = np.zeros(len(lists) + 1, np.int32)
    begin[1:] = np.cumsum([len(d) for d in lists])
    xy = np.ascontiguousarray(np.concatenate(lists), float)
    opt = mpe.MpeRigInitOptions(**{k: int(v) for k, v in options.items()})
    rec = np.zeros(1, mpe.RESULT_DTYPE)
    match = np.full((len(cameras), len(mk)), 0xFFFFFFFF, np.uint32)
    info = np.zeros(1, mpe.RIG_INIT_INFO_DTYPE)
    tv, ta = np.ascontiguousarray(tol_v, float), np.ascontiguousarray(tol_a, float)
    host.host_rig_single(cams, len(cameras), _ptr(mk), len(mk), C.byref(opt), _ptr(begin), _ptr(xy), _ptr(tv), _ptr(ta), _ptr(rec),
                         _ptr(match), _ptr(info))
    return rec[0], match, info[0]


def translated(problem, owner, b, rec, match, info):
    """What round b must be, made from the single-body answer (rec, match, info) over the lists `owner` leaves: the
    indices that name detections translated to the caller's lists, the match words behind MAX_MARKERS.  -> (record bytes,
    match (n_cam, MAX_MARKERS), info bytes, the owner map behind the round's claims)"""
    _, keep = WB.free_lists(problem, owner)
    n_cam, n_mk = match.shape
    m = np.zeros((n_cam, mpe.MAX_MARKERS), np.uint32)
    for c in range(n_cam):
        nz = match[c] != 0
        m[c, :n_mk][nz] = keep[c][match[c][nz].astype(np.int64) - 1] + 1
    info = info.copy()
    if info["camera"] >= 0:
        info["detection"] = keep[int(info["camera"])][info["detection"]]
    owner = [o.copy() for o in owner]
    if int(info["reason"]) == 0:
        for c in range(n_cam):
            owner[c][m[c][m[c] != 0].astype(np.int64) - 1] = b
    return rec.tobytes(), m, info.tobytes(), owner


def check_rounds_against_single(problem, got, run_single, what=None):
    """every (body) record, info and match of `got` = (rec, match, info, owner) equals, byte for byte with indices
    translated, what run_single(markers, lists, options) -> (rec, match, info) returns for the lists filtered HERE"""
    rec, match, info, owner_got = got
    owner = WB.entry_owner(problem)
    find = problem.get("find")
    for b, (markers, _) in enumerate(problem["bodies"]):
        if find is not None and not find[b]:
            assert int(info[b]["reason"]) == WB.NOT_ASKED and not match[b].any() and int(rec[b]["status"]) == 1, (what, b)
            continue
        lists, _ = WB.free_lists(problem, owner)
        r, m, i = run_single(markers, lists, WB.body_options(problem, b))
        rb, mb, ib, owner = translated(problem, owner, b, r, m, i)
        assert rec[b].tobytes() == rb, (what, b)
        assert np.array_equal(match[b], mb), (what, b, match[b], mb)
        assert info[b].tobytes() == ib, (what, b, info[b], i)
    for c in range(len(owner)):
        assert np.array_equal(np.asarray(owner_got[c], np.int64), owner[c]), (what, c)


@pytest.fixture(scope="module")
def drawn():
    return WB.drawn_problems()


def test_drawn_problems_against_the_witness(host, drawn):
    problems, redraws = drawn
    assert len(problems) == 60 and redraws <= len(problems) // 10, redraws
    reasons, shapes = {}, {}
    for k, p in enumerate(problems):
        rec, match, info, owner = host_bodies(host, p["problem"])
        WB.check_against_witness(rec, match, info, owner, p["problem"], k, ws=p["ws"])
        for w in p["ws"][0]:
            reasons[w["reason"]] = reasons.get(w["reason"], 0) + 1
        key = (len(p["problem"]["cameras"]), len(p["problem"]["bodies"]))
        shapes[key] = shapes.get(key, 0) + 1
    record = WB.recorded()["drawn"]
    assert len(record) == len(problems)
    for k, p in enumerate(problems):
        assert record[k]["attempt"] == p["attempt"] and WB.same_witness(WB.unpack(record[k]), p["ws"]), k
    absent = sum(1 for p in problems if not all(p["present"]))
    print("re-drawn: %d of %d; a body absent in %d; reasons: %s; (cameras, bodies): %s"
          % (redraws, len(problems), absent, sorted(reasons.items()), sorted(shapes.items())))
    assert {0, 6} <= set(reasons) and {1, 2, 3} == {nc for nc, _ in shapes}, (reasons, shapes)
    # four rounds against the witness, more than once, and an M8 that is FOUND
    assert sum(n for (_, nb), n in shapes.items() if nb == 4) >= 3 and sum(n for (_, nb), n in shapes.items() if nb == 3) >= 2, shapes
    assert any(w["reason"] == 0 and len(M) == 8 for p in problems for w, (M, _) in zip(p["ws"][0], p["problem"]["bodies"]))


def test_the_exact_shapes(host):
    shapes, redraws = WB.shapes()
    assert redraws <= 1, redraws
    assert [s["name"] for s in shapes] == [name for name, _ in WB.SHAPES]
    record = WB.recorded()["shapes"]
    assert len(record) == len(shapes)
    for r, s in zip(record, shapes):
        rec, match, info, owner = host_bodies(host, s["problem"])
        WB.check_against_witness(rec, match, info, owner, s["problem"], s["name"], ws=s["ws"])
        WB.check_expectation(s)
        assert r["attempt"] == s["attempt"] and WB.same_witness(WB.unpack(r), s["ws"]), s["name"]


def test_a_list_of_64_with_both_ends_claimed(host):
    made = WB.claimed_ends()
    rec, match, info, owner = host_bodies(host, made[0])
    WB.check_claimed_ends(rec, match, info, owner, made)


def test_the_bodies_in_reverse_order_give_the_mirrored_owner_map(host):
    s = [x for x in WB.shapes(record=WB.recorded()["shapes"])[0] if x["name"] == "identical"][0]
    a = host_bodies(host, s["problem"])
    b = host_bodies(host, WB.reversed_problem(s["problem"]))
    # identical bodies: the same searches in the same order, so round k owns the same points — which is, under the bodies'
    # ORIGINAL names (round k of the reversed call is body 1 - k), the mirrored map
    for oa, ob in zip(a[3], b[3]):
        named = np.where(ob >= 0, 1 - ob, ob)
        assert np.array_equal(named, np.where(oa >= 0, 1 - oa, oa)) and {0, 1} <= set(oa.tolist())
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))
    # bodies that differ: M5 in front of M4 and M4 in front of M5 on the points of one M5 and one M4 body
    made = WB._one_camera(np.random.default_rng([WB.SHAPE_SEED, 65]), ["M5", "M4"], strays=2)
    fwd = host_bodies(host, made[0])
    assert [int(i["reason"]) for i in fwd[2]] == [0, 0] and np.array_equal(fwd[3][0], made[1][0])
    rev = host_bodies(host, WB.reversed_problem(made[0]))
    check_rounds_against_single(WB.reversed_problem(made[0]), rev,
                                lambda M, lists, o: host_single(host, made[0]["cameras"], M, lists, made[0]["tol_vote"],
                                                                made[0]["tol_accept"], o), "reversed")


def test_one_body_is_the_single_body_run(host, single, drawn):
    """n_bodies == 1 without claimed_in: the bytes of the single-body host run (tests/test_rig_init_host.py's build)"""
    n = 0
    for k, p in enumerate(drawn[0]):
        pr = p["problem"]
        if len(pr["bodies"]) != 1:
            continue
        rec, match, info, owner = host_bodies(host, pr)
        M = pr["bodies"][0][0]
        r, m, i = TI.host_init(single, (pr["cameras"], M, pr["dets"], pr["tol_vote"], pr["tol_accept"]), **WB.body_options(pr, 0))
        assert rec[0].tobytes() == r.tobytes() and info[0].tobytes() == i.tobytes(), k
        assert np.array_equal(match[0][:, :len(M)], m) and not match[0][:, len(M):].any(), k
        n += 1
    assert n >= 10, n


def test_a_round_is_the_single_body_run_over_the_filtered_lists(host, drawn):
    shapes, _ = WB.shapes(record=WB.recorded()["shapes"])
    for k, p in enumerate([q for q in drawn[0] if len(q["problem"]["bodies"]) > 1][:16] + drawn[0][-len(WB.SPREAD):] + shapes):
        pr = p["problem"]
        got = host_bodies(host, pr)
        check_rounds_against_single(pr, got, lambda M, lists, o: host_single(host, pr["cameras"], M, lists, pr["tol_vote"],
                                                                             pr["tol_accept"], o), p.get("name", k))


# the parity problems this tier runs (the host build does 0.5 M items a second): those of up to 300 000 items and the
# four-body ones of up to 550 000; the GPU tier runs all
PARITY_ITEMS, PARITY_ITEMS_FOUR = 300000, 550000


def test_the_full_range_of_bodies_without_the_witness(host):
    """1 - 4 bodies out of {M4, M5, M5, M8} with M8 in full view, no item budget (witness_rig_bodies.parity_problems): every
    round is the single-body run over the lists filtered here, and the block count of the unfiltered lists does not show"""
    problems = [p for p in WB.parity_problems()
                if p["items"] <= (PARITY_ITEMS_FOUR if len(p["problem"]["bodies"]) == 4 else PARITY_ITEMS)]
    n_bodies, m8_found, fourth_found = {}, 0, 0
    for k, p in enumerate(problems):
        pr = p["problem"]
        got = host_bodies(host, pr)
        check_rounds_against_single(pr, got, lambda M, lists, o: host_single(host, pr["cameras"], M, lists, pr["tol_vote"],
                                                                             pr["tol_accept"], o), k)
        exact = host_bodies(host, pr, blocks=1)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:3], exact[:3])), k
        assert all(np.array_equal(x, y) for x, y in zip(got[3], exact[3])), k
        n_bodies[len(pr["bodies"])] = n_bodies.get(len(pr["bodies"]), 0) + 1
        m8_found += sum(int(i["reason"]) == 0 and len(M) == 8 for i, (M, _) in zip(got[2], pr["bodies"]))
        fourth_found += int(len(pr["bodies"]) == 4 and int(got[2][3]["reason"]) == 0)
    print("bodies: %s; an M8 found %d times, a fourth body %d times" % (sorted(n_bodies.items()), m8_found, fourth_found))
    assert set(n_bodies) == {1, 2, 3, 4} and n_bodies[4] >= 3 and m8_found >= 3 and fourth_found >= 1, (n_bodies, m8_found, fourth_found)


def test_the_block_count_of_the_unfiltered_lists_does_not_show(host, drawn):
    shapes, _ = WB.shapes(record=WB.recorded()["shapes"])
    for k, p in enumerate(drawn[0][:20] + drawn[0][-len(WB.SPREAD):] + shapes):
        a = host_bodies(host, p["problem"], blocks=0)
        b = host_bodies(host, p["problem"], blocks=1)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])), k
        assert all(np.array_equal(x, y) for x, y in zip(a[3], b[3])), k


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", *flags, "-DRIG_PEEL_HOST_MAIN", *TI.extract(tmp_path), SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "rig_peel_host ok:" in r.stdout, r.stdout
    return r.stdout


def test_rig_peel_on_the_host_stand_alone(tmp_path):
    out = _build_and_run(tmp_path, "rig_peel_host", ["-O2"])
    assert "10 scenes, 20 bodies found" in out, out


def test_rig_peel_on_the_host_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "rig_peel_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                   "-fno-omit-frame-pointer"])


C_USER = r"""
#include <stdio.h>
#include "mpe.h"
int main(void) {
  mpe_rig_init_options one, rig;
  mpe_rig_body body;
  int (*batch)(mpe_handle*, const mpe_rig_camera*, int, const mpe_rig_body*, int, const int*, const double*, const uint8_t*,
               const uint8_t*, const double*, const double*, int, mpe_result*, uint32_t*, mpe_rig_init_info*, int8_t*) =
      mpe_rig_init_bodies_batch;
  int (*trackers)(mpe_tracker* const*, int, int, const double*, const int*, const int*, double, mpe_result*, uint32_t*,
                  mpe_rig_init_info*, int8_t*) = mpe_rig_init_bodies_trackers;
  mpe_rig_init_bodies_default_options(&one, 1, 5);
  mpe_rig_init_bodies_default_options(&rig, 3, 5);
  body.n_markers = 0;
  printf("%d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(body), MPE_MAX_BODIES, one.max_rounds, one.min_rows, one.min_markers,
         one.min_margin, rig.max_rounds, rig.min_rows, rig.min_markers, rig.min_margin, (batch && trackers) + body.n_markers);
  return 0;
}
"""


def test_bodies_declarations_are_c99_exported_and_sized(tmp_path):
    mpe.build_library()
    lib = mpe.load_library()
    names = {"mpe_rig_init_bodies_batch", "mpe_rig_init_bodies_trackers", "mpe_rig_init_bodies_default_options"}
    assert names <= set(mpe.exported_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", mpe.library_path()], text=True)
    assert names <= set(re.findall(r" T (mpe_[a-z0-9_]+)", out))
    src = tmp_path / "rig_bodies_user.c"
    src.write_text(C_USER)
    exe = str(tmp_path / "rig_bodies_user")
    libdir = os.path.dirname(mpe.library_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe, "-L", libdir, "-lmpe_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert got == [str(C.sizeof(mpe.MpeRigBody)), "16", "2", "5", "5", "0", "2", "6", "4", "0", "1"], got
    assert C.sizeof(mpe.MpeRigBody) == 24 and mpe.MAX_BODIES == 16
    lib.mpe_rig_init_bodies_default_options(None, 1, 5)      # (ignored)
    csrc = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")
    assert "mpe_rig_peel.h" in open(os.path.join(csrc, "Makefile")).read()
    assert '#include "mpe_rig_peel.h"' in open(os.path.join(csrc, "mpe_rig_peel.hip")).read()


def test_the_refusals_that_need_no_device():
    mpe.build_library()
    lib = mpe.load_library()
    ARG, UNSUPPORTED = -1, -3
    cams = mpe.binding.pack_rig_cameras([(np.eye(3), np.eye(4))])
    mk = np.ascontiguousarray(synth.M5)
    tol = np.array([3.0])
    rec = np.zeros(4, mpe.RESULT_DTYPE)

    def call(n_cam=1, bodies=((mk, None),), n_bodies=None, begin=(0, 5), xy=None, claimed=None, find=None, tv=tol, ta=tol, n=1,
             out=rec, cameras=cams, no_bodies=False):
        packed, keep = mpe.binding.pack_rig_bodies(lib, list(bodies), n_cam)
        b = np.array(begin, np.int32)
        xy = np.zeros((max(1, int(b[-1])), 2)) if xy is None else xy
        cl = None if claimed is None else np.ascontiguousarray(claimed, np.uint8)
        fi = None if find is None else np.ascontiguousarray(find, np.uint8)
        return lib.mpe_rig_init_bodies_batch(None, cameras, n_cam, None if no_bodies else packed, len(bodies) if n_bodies is None else n_bodies,
                                             b.ctypes.data_as(C.POINTER(C.c_int)), xy.ctypes.data_as(C.POINTER(C.c_double)),
                                             _ptr(cl), _ptr(fi), tv.ctypes.data_as(C.POINTER(C.c_double)),
                                             ta.ctypes.data_as(C.POINTER(C.c_double)), n, None if out is None else out.ctypes.data,
                                             None, None, None)

    assert call(n=0) == 0                                     # n_problems == 0: MPE_OK
    assert call() == ARG                                      # everything in order but the handle
    assert call(n=-1) == ARG and call(cameras=None) == ARG and call(no_bodies=True) == ARG and call(out=None) == ARG
    assert call(n_bodies=0) == ARG and call(bodies=((mk, None),) * 17) == ARG
    assert call(n_cam=0) == ARG and call(n_cam=17) == ARG
    assert call(bodies=((np.zeros((17, 3)), None),)) == ARG
    for bad in (dict(max_rounds=0), dict(max_rounds=5), dict(min_rows=2), dict(min_markers=0), dict(min_margin=-1)):
        assert call(bodies=((mk, None), (mk, bad))) == ARG, bad
    assert call(tv=np.array([0.0])) == ARG and call(ta=np.array([np.nan])) == ARG
    assert call(begin=(-1, 3)) == ARG and call(begin=(3, 2)) == ARG
    assert call(begin=(0, 65)) == UNSUPPORTED
    # one list of 64 with 6 markers: 5.0 M items; with 5 markers 2.5 M are admitted (the handle is what is missing then)
    six = np.vstack([synth.M5, [[0.1, 0.1, 0.1]]])
    assert call(bodies=((mk, None), (six, None)), begin=(0, 64)) == UNSUPPORTED
    assert call(bodies=((mk, None),), begin=(0, 64)) == ARG
    # ... counted over the lists claimed_in leaves, and only for a body that is asked for
    claimed = np.zeros(64, np.uint8)
    claimed[:8] = 1                                          # 56 points: C(56, 3) * 120 = 3.3 M
    assert call(bodies=((six, None),), begin=(0, 64), claimed=claimed) == ARG
    assert call(bodies=((mk, None), (six, None)), begin=(0, 64), find=[1, 0]) == ARG
    tr = lib.mpe_rig_init_bodies_trackers
    assert tr(None, 1, 1, None, None, None, 2.0, None, None, None, None) == ARG


# ---- the measurement behind INTEGRATION.md's table ----------------------------------------------------------------

def _scene(seed, names, strays=0, noise=0.0, present=None):
    return WB._one_camera(np.random.default_rng([20261021, seed]), names, strays=strays, noise=noise, present=present)


def _true_body(T, T_true, taken=()):
    for k, Tk in enumerate(T_true):
        if Tk is not None and k not in taken and np.linalg.norm(T[:3, 3] - Tk[:3, 3]) < 0.02:
            return k
    return None


def test_two_bodies_in_view_histogram_search_and_peel(host, orc):
    """The two experiments behind INTEGRATION.md's table, as counts of seeds.  (a) the reference's histogram search
    (oracle.solve_bruteforce; the `synth` camera's K, exact projections, blobs at least 12 px apart, 40 seeds) with two
    bodies in view: does the first body get a pose that is a true body's, and a second search on what the first left the
    other's.  (b) the peel over the host build (one camera, identity extrinsic, 0.1 px noise, the bodies' defaults, 30
    seeds): every body found, each on another true body within 2 cm; and one body more than is in view asked for.
    Asserted: the direction — the peel finds every body on more seeds than the histogram search finds both —, and that no
    absent body gets a pose."""
    params = orc.make_params()
    K = WB.W.exact_camera()[0]
    table = {}
    for names in (["M5", "M5"], ["M5", "M4"], ["M4", "M5"], ["M4", "M4"]):
        first = both = 0
        for seed in range(40):
            pr, truth, T_true, _ = _scene(seed, names)
            det = pr["dets"][0]
            r = orc.solve_bruteforce(det, WB.KINDS[names[0]], K, params)
            k0 = _true_body(r["T"], T_true) if r["status"] == 0 else None
            if k0 is None:
                continue
            first += 1
            rest = det[truth[0] != k0]
            r2 = orc.solve_bruteforce(rest, WB.KINDS[names[1]], K, params)
            both += int(r2["status"] == 0 and _true_body(r2["T"], T_true, (k0,)) is not None)
        table[" + ".join(names)] = (first, both)
    peel = {}
    absent_with_pose = 0
    for names, strays in ((["M5", "M5"], 0), (["M5", "M5", "M5"], 0), (["M5", "M5"], 4), (["M4", "M4"], 0), (["M5", "M4"], 0)):
        found = 0
        for seed in range(30):
            pr, truth, T_true, _ = _scene(100 + seed, names, strays=strays, noise=0.1)
            rec, match, info, owner = host_bodies(host, pr)
            taken = []
            for b in range(len(names)):
                k = _true_body(rec[b]["T"].reshape(4, 4), T_true, taken) if rec[b]["status"] == 0 else None
                if k is not None:
                    taken.append(k)
            found += int(len(taken) == len(names))
        peel[" + ".join(names) + (" + %d strays" % strays if strays else "")] = found
    for names, present, strays in ((["M5", "M5"], [True, False], 4), (["M5", "M5", "M5"], [True, True, False], 8),
                                   (["M5", "M5"], [True, False], 8), (["M5", "M5", "M5"], [True, True, False], 4)):
        for seed in range(30):
            pr, truth, T_true, _ = _scene(200 + seed, names, strays=strays, noise=0.1, present=present)
            rec, match, info, owner = host_bodies(host, pr)
            absent_with_pose += int(rec[len(names) - 1]["status"] == 0)
    print("histogram search, of 40 seeds (first body gets a pose, both get one):")
    for k, v in table.items():
        print("  %-10s %2d %2d" % (k, v[0], v[1]))
    print("peel over the host build, of 30 seeds (all bodies found, each on another true body):")
    for k, v in peel.items():
        print("  %-22s %2d" % (k, v))
    print("an absent body got a pose on %d of 120 seeds" % absent_with_pose)
    assert absent_with_pose == 0
    assert min(peel.values()) > max(both for _, both in table.values()), (peel, table)
