"""GPU: the map query (dsp_map_query) and the map alignment (dsp_map_align) where their index paths change with size -- more than 256 objects
in a chunk (the second LDS stage of k_query_count / k_query_fill), chunks that start inside an object and go on over hundreds more, objects
without candidates between objects that have some, the reduced pass size from 8193 objects on, and more than 65 535 hypotheses (the
gridDim.y split of launch_align_gram).

Expected values: the float32 restatements tests/query_ref.py and tests/align_ref.py composed with the device's own decoder rows, bit for
bit, as in tests/test_gpu_map_query.py and tests/test_gpu_map_align.py; the chunk geometry from dsp_debug_query_plan, which
tests/test_query_plan_host.py holds to the plain statement of the plan; and, in test_large_map_against_float64, the operation stated in
plain float64 (query_ref.expected64) with tolerances from the number formats.  What each test measured is printed and appended to the
parity log; profiles/map_scale.md has the figures of one run.
"""
import numpy as np
import pytest

import align_ref as A
import query_ref as Q
import test_gpu_map_align as TA
from conftest import parity_log
from dsp_slam_amd import engine as E, _lib as L
from test_gpu_map_query import _bits_equal, _in_ball, _same
from test_query_plan_host import host_plan, pass_pts

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
ALL4 = ("obj", "dist", "bound", "normal")
T_TRUE = TA.T_TRUE


@pytest.fixture(scope="module")
def eng(oracle_decoder):
    e = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)
    yield e
    e.close()


def lattice(rng, n_obj, pitch):
    """n_obj objects at the nodes of a cubic lattice of side ceil(n_obj^(1/3)), random rotations, scales in 0.6 .. 1.2 (the unit spheres of
    neighbours overlap at pitch 1.1), codes uniform in -0.3 .. 0.3 -> poses (n_obj, 4, 4) float32, list of codes."""
    side = 1
    while side ** 3 < n_obj:
        side += 1
    k = np.arange(n_obj)
    centres = np.stack([k % side, (k // side) % side, k // (side * side)], 1) * float(pitch)
    t = Q.sim3(Q.random_rotations(rng, n_obj), rng.uniform(0.6, 1.2, n_obj), centres)
    return t, list(rng.uniform(-0.3, 0.3, (n_obj, 64)).astype(F32))


def inside_points(rng, t, owners, r=0.97):
    """one world point per entry of owners, within r of the centre of that object's unit sphere (object frame)"""
    p = _in_ball(rng, len(owners), r)
    t64 = t[np.asarray(owners)].astype(F64)
    return (np.einsum("nij,nj->ni", t64[:, :3, :3], p) + t64[:, :3, 3]).astype(F32)


def clutter(rng, n):
    return (rng.uniform(-1.0, 1.0, (n, 3)) + 500.0).astype(F32)


def chunk_rows(eng, rows, call):
    """call() with the handle's chunk budget at `rows`, restored afterwards"""
    lib = L.load()
    assert lib.dsp_debug_query_chunk_rows(eng._h, rows) == 0
    try:
        return call()
    finally:
        assert lib.dsp_debug_query_chunk_rows(eng._h, 0) == 0


def same_bytes(a, b, keys):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- the scenes: computed once, never modified -------------------------------------------------------------------------------------------
_S600, _S257, _S64, _ALIGN = {}, {}, {}, {}


def scene600(eng):
    """600 objects, 1500 shuffled points: 1400 inside the spheres of chosen owners (never objects 0 to 2 nor any o with o % 5 == 1; 300 of
    them in object 300, 130 in object 599), 100 far from everything; with the restatement's expected result."""
    if not _S600:
        rng = np.random.default_rng(60)
        t, codes = lattice(rng, 600, 1.1)
        allowed = np.array([o for o in range(3, 600) if o % 5 != 1])
        owners = np.concatenate([np.full(300, 300), np.full(130, 599), rng.choice(allowed, 970)])
        pts = np.concatenate([inside_points(rng, t, owners), clutter(rng, 100)])[rng.permutation(1500)]
        exp = Q.expected(eng, t, codes, pts, with_normals=True)
        cnt = exp["inside"].sum(1)
        some = np.flatnonzero(cnt > 0)
        empty = np.flatnonzero(cnt == 0)
        between = empty[(empty > some[0]) & (empty < some[-1])]
        neg = int((exp["dist"] < 0).sum())
        fig = dict(rows=int(cnt.sum()), empty=int(empty.size), empty_between=int(between.size), rows_300=int(cnt[300]), rows_599=int(cnt[599]),
                   per_point=float(cnt.sum() / 1500.0), most=int(exp["inside"].sum(0).max()), negative=neg)
        print("scene600:", fig)
        parity_log(case="map_scale_scene600", **fig)
        assert empty.size >= 10 and between.size >= 1
        assert (cnt[257:] > 64).any() and cnt.sum() >= 2 * 1500 and neg >= 300
        _S600.update(t=t, codes=codes, pts=pts, exp=exp, cnt=cnt.astype(np.int32), fig=fig)
    return _S600


def scene257(eng):
    """257 objects -- one object into the second LDS stage -- and 500 points, some of them forced into objects 0, 255 and 256"""
    if not _S257:
        rng = np.random.default_rng(257)
        t, codes = lattice(rng, 257, 1.1)
        owners = np.concatenate([np.full(20, 0), np.full(30, 255), np.full(70, 256), rng.choice(257, 350)])
        pts = np.concatenate([inside_points(rng, t, owners), clutter(rng, 30)])[rng.permutation(500)]
        exp = Q.expected(eng, t, codes, pts, with_normals=True)
        cnt = exp["inside"].sum(1)
        assert cnt[0] > 0 and cnt[255] > 0 and cnt[256] > 64 and (exp["obj"] == 256).sum() >= 20
        _S257.update(t=t, codes=codes, pts=pts, exp=exp, cnt=cnt.astype(np.int32))
    return _S257


# ---- a. 600 objects against the restatement ----------------------------------------------------------------------------------------------
def test_600_objects_are_the_restatement_bit_for_bit(eng):
    s = scene600(eng)
    res = eng.query_map(s["t"], s["codes"], s["pts"], normals=True)
    st = eng.query_stats()
    _same(res, s["exp"], keys=ALL4)
    _same(eng.query_map(s["t"], s["codes"], s["pts"]), s["exp"])
    cnt = s["cnt"].astype(np.int64)
    chunks = host_plan(cnt, 0)[0]
    # one chunk from the first object that has candidates to the last object of the map: both LDS stage loops run three times
    assert chunks.shape[0] == 1 and chunks[0, 1] > 512
    assert st == {"rows": int(cnt.sum()), "tiles": int((-(-cnt // 64)).sum()), "chunks": 1, "passes": 1}
    assert eng.query_stats() == st


@pytest.mark.parametrize("rows", [70, 1000])
def test_600_objects_chunked_are_the_unchunked_bytes(eng, rows):
    s = scene600(eng)
    whole = eng.query_map(s["t"], s["codes"], s["pts"], normals=True)

    def call():
        r = eng.query_map(s["t"], s["codes"], s["pts"], normals=True)
        return r, eng.query_stats(), eng.query_map(s["t"], s["codes"], s["pts"])
    chunked, st, plain = chunk_rows(eng, rows, call)
    same_bytes(chunked, whole, ALL4)
    same_bytes(plain, whole, ALL4[:3])
    _same(chunked, s["exp"], keys=ALL4)
    chunks, base, tiles = host_plan(s["cnt"], rows)
    assert st["chunks"] == chunks.shape[0] == -(-int(s["cnt"].sum()) // rows) and st["tiles"] == tiles.shape[0] and st["rows"] == int(s["cnt"].sum())
    inside_start = base[np.cumsum(chunks[:, 1]) - chunks[:, 1]] < 0             # the chunk starts inside its first object
    print("chunk rows %d: %d chunks, %d start inside an object, most objects in a chunk %d" % (rows, chunks.shape[0], inside_start.sum(), chunks[:, 1].max()))
    assert inside_start.any()
    if rows == 1000:
        assert ((chunks[:, 0] > 0) & (chunks[:, 1] > 256)).any()


def test_257_objects_are_the_restatement_bit_for_bit(eng):
    s = scene257(eng)
    res = eng.query_map(s["t"], s["codes"], s["pts"], normals=True)
    st = eng.query_stats()
    _same(res, s["exp"], keys=ALL4)
    _same(eng.query_map(s["t"], s["codes"], s["pts"]), s["exp"])
    chunks = host_plan(s["cnt"], 0)[0]
    assert chunks.tolist() == [[0, 257, int(s["cnt"].sum()), st["tiles"]]] and st["chunks"] == 1     # 256 objects in the first stage, 1 in the second
    chunked, st70 = chunk_rows(eng, 70, lambda: (eng.query_map(s["t"], s["codes"], s["pts"], normals=True), eng.query_stats()))
    same_bytes(chunked, res, ALL4)
    assert st70["chunks"] == host_plan(s["cnt"], 70)[0].shape[0] > 1


# ---- b. the same scene against plain float64 ---------------------------------------------------------------------------------------------
def test_large_map_against_float64(eng, oracle_decoder):
    """Every point of the 600-object scene against the operation in float64 (query_ref.expected64): p_o = T^-1 p, dist = s sdf64(code, p_o),
    winner = argmin, n = R g / |g|, bound = min (|p_o| - 1) s.  No point is excluded from obj, dist or bound.

    dist: tol = s (TAU_DEC + 2 |g64| delta) per row.  TAU_DEC = 5e-6 is what tests/test_gpu_decoders.py asserts for the fp32 decoder
    against the float64 oracle AT THE SAME POINT; the device decodes at the float32 p_o of the restatement, delta = |p_o32 - p_o64| away, which
    moves the value by |g| delta to first order; the factor 2 covers the change of g over that step and s32 against s64 (2^-24 relative).
    winner: the device chose w with d32[w] <= d32[m] for the float64 minimum m, so d64[w] <= d64[m] + tol[w] + tol[m] -- "2 tol" with each
    row's own tolerance.  The scene has no float64 near-tie (asserted on the float64 values alone), so this identifies the winner.

    bound: |bound - bound64| <= 4 eps32 (|t_ow| + |p| / s) s, eps32 = 2^-23.  to_object computes each coordinate as
    fma(r2, z, fma(r1, y, fma(r0, x, t))): three fused multiply-adds, one rounding each, on entries r, t that are themselves float64 values
    rounded once -- four roundings of relative size eps32 / 2 applied to quantities bounded by A = sum_j |r_j p_j| + |t| <= |p| / s + |t_ow|,
    so |p_o32 - p_o64| <= 2 eps32 A.  The norm (three squares, two sums: 3 roundings in |p_o|^2, halved by the root), the root, the
    subtraction of 1 and the product with s add at most 4.5 roundings of eps32 / 2 relative to |p_o| <= A: 2.25 eps32 A.  Together 4.25 eps32
    A s; 4 is kept, as the roundings cannot all take their worst value in one direction (the measured worst ratio is in profiles/map_scale.md).
    The minimum over objects may sit at another object in float32 than in float64: the tolerance is the largest one among the objects whose
    float64 bound lies within twice the largest tolerance of the minimum (query_ref.expected64).

    normal: against R g64 / |g64| of the device's winner.  Rows whose gradient differs between the two sides of a ReLU kink within fp32
    round-off (the oracle's flipped-mask gradient, with the point's own rounding delta in the band) have no single float64 answer and are
    left out; their share must stay below 1 %.  For the rest the allowance per component is 4 x (1e-5 max(1, |g|max) / |g64|): the
    per-entry gradient bound tests/test_gpu_decoders.py asserts, carried to the unit vector by 1 / |g64|, times 4 for the three components
    that enter each entry of the normalised vector (sqrt(3) in norm) and the roundings of the rotation and the normalisation."""
    s = scene600(eng)
    exp = s["exp"]
    if not _S64:
        _S64.update(Q.expected64(oracle_decoder, s["t"], s["codes"], s["pts"], exp))
    r64 = _S64
    n_pts = s["pts"].shape[0]
    res = eng.query_map(s["t"], s["codes"], s["pts"], normals=True)
    ob, pt, d, tol = r64["obj"], r64["pt"], r64["d"], r64["tol"]
    assert np.array_equal(ob, exp["rows"]["obj"]) and np.array_equal(pt, exp["rows"]["pt"])
    # containment: a winner exactly where the restatement has a candidate
    has = exp["inside"].any(0)
    assert np.array_equal(res["obj"] >= 0, has) and np.all(np.isposinf(res["dist"][~has])) and np.all(res["normal"][~has] == 0)
    hit = np.flatnonzero(has)
    row_of = np.full(exp["inside"].shape, -1, np.int64)
    row_of[ob, pt] = np.arange(ob.size)
    w = row_of[res["obj"][hit], hit]
    assert (w >= 0).all()                                   # the winner is one of the point's candidates
    # the float64 minimum of every point and the runner-up
    order = np.lexsort((d, pt))
    first = np.ones(order.size, bool)
    first[1:] = pt[order][1:] != pt[order][:-1]
    m = order[first]
    assert np.array_equal(pt[m], hit)
    second = np.full(n_pts, np.inf)
    nxt = np.flatnonzero(~first)
    nxt = nxt[first[nxt - 1]]                               # the entry right behind a point's minimum
    second[pt[order][nxt]] = d[order][nxt]
    second_tol = np.zeros(n_pts)
    second_tol[pt[order][nxt]] = tol[order][nxt]
    near_tie = int((second[hit] - d[m] <= tol[m] + second_tol[hit]).sum())      # from the float64 values alone
    margin = tol[w] + tol[m]
    # dist
    err = np.abs(res["dist"][hit].astype(F64) - d[w])
    ratio_d = float((err / tol[w]).max())
    # bound
    with np.errstate(invalid="ignore"):
        berr = np.where(np.isinf(r64["bound"]) & np.isinf(res["bound"]), 0.0, np.abs(res["bound"].astype(F64) - r64["bound"]))
    ratio_b = float((berr / r64["bound_tol"]).max())
    # normals
    flip_rows = (r64["g_flip"] != r64["g"]).any(1)
    share = float(flip_rows.mean())
    keep = ~flip_rows[w]
    gmax = float(np.abs(r64["g"]).max())
    allow = 4.0 * 1e-5 * max(1.0, gmax) / np.sqrt((r64["g"][w] ** 2).sum(1))
    nerr = np.abs(res["normal"][hit].astype(F64) - r64["n"][w]).max(1)
    ratio_n = float((nerr[keep] / allow[keep]).max())
    fig = dict(points=int(n_pts), rows=int(ob.size), near_ties=near_tie, dist_ratio=ratio_d, dist_err=float(err.max()), bound_ratio=ratio_b,
               bound_err=float(berr.max()), normal_ratio=ratio_n, normal_err=float(nerr[keep].max()), flipped_rows=int(flip_rows.sum()),
               flipped_share=share, flipped_winners=int((~keep).sum()), gmax=gmax, delta_max=float(r64["delta"].max()),
               winners_not_float64_minimum=int((w != m).sum()))
    print("float64:", fig)
    parity_log(case="map_scale_float64", **fig)
    assert near_tie == 0
    assert np.all(err <= tol[w])
    assert np.all(d[w] <= d[m] + margin)
    assert np.all(berr <= r64["bound_tol"])
    assert share <= 0.01
    assert np.all(nerr[keep] <= allow[keep])


# ---- c. alignment on the large map -------------------------------------------------------------------------------------------------------
def align600(eng):
    if not _ALIGN:
        s = scene600(eng)
        rng = np.random.default_rng(61)
        world = s["pts"][:300].astype(F64)                  # the scene's points are shuffled: any 300 are a sample of all kinds
        codes = s["codes"]
        hyp = np.stack([T_TRUE, A.offset_pose(rng, T_TRUE, 5.0, 0.05, world[np.abs(world).max(1) < 100].mean(0))])
        w = rng.uniform(0.0, 2.0, 300).astype(F32)
        w[rng.permutation(300)[:20]] = 0.0
        _ALIGN.update(t=s["t"], codes=codes, map=A.Map(s["t"], codes), decode=TA._decoder(eng, codes), pts=TA._to_sensor(T_TRUE, world), hyp=hyp, w=w)
    return _ALIGN


@pytest.mark.parametrize("weighted", [False, True])
def test_alignment_on_the_large_map(eng, weighted):
    a = align600(eng)
    w = a["w"] if weighted else None
    kw = dict(weights=w, iterations=1, trans_tol=0.0, rot_tol=0.0)
    res = TA._align(eng, a, a["hyp"], **kw)
    st = eng.align_stats()
    rows = 0
    for k in range(2):
        ev = TA._ref_eval(a, a["hyp"][k], None, w)
        TA._record_is(res, k, ev)
        assert np.array_equal(res["obj"][k], ev["obj"]) and TA._same32(res["dist"][k], ev["dist"]), k
        ins = Q.candidates(a["map"].rt, a["map"].s, ev["pw"])[1]
        rows += int(ins.sum())
        # the scene: support, winners on both sides of object 256, objects without candidates between objects that have some
        cnt = ins.sum(1)
        some = np.flatnonzero(cnt)
        assert ev["n_used"] >= 30 and (ev["obj"] > 256).sum() >= 30 and ((ev["obj"] >= 0) & (ev["obj"] < 256)).sum() >= 30
        assert (cnt[some[0]:some[-1]] == 0).sum() >= 10 and some[-1] - some[0] > 512
    assert st["rows"] == rows and st["chunks"] == 1 and st["evaluations"] == 1
    chunked, st70 = chunk_rows(eng, 70, lambda: (TA._align(eng, a, a["hyp"], **kw), eng.align_stats()))
    assert TA._bytes(chunked) == TA._bytes(res)
    assert st70["rows"] == rows and st70["chunks"] == -(-rows // 70)


# ---- d. the reduced pass size: 8200 objects ------------------------------------------------------------------------------------------------
def test_8200_objects_take_the_reduced_pass(eng):
    rng = np.random.default_rng(8200)
    n_obj = 8200
    t, codes = lattice(rng, n_obj, 1.1)
    P = pass_pts(n_obj)
    assert P == 130944 < 1 << 17
    n = P + 200
    pts = clutter(rng, n)
    fixed = np.concatenate([np.arange(100), np.arange(P - 100, P + 100), np.arange(n - 100, n)])
    rest = np.setdiff1d(np.arange(n), fixed)
    S = np.sort(np.concatenate([fixed, rng.choice(rest, 200, replace=False)]))
    assert S.size == 600 and np.unique(S).size == 600
    owners = np.concatenate([np.arange(0, 256, 8), [255, 256, 257], np.arange(8191, 8200), rng.choice(n_obj, 600 - 32 - 3 - 9)])
    owners = owners[rng.permutation(600)]
    pts[S] = inside_points(rng, t, owners)
    exp = Q.expected(eng, t, codes, pts[S], with_normals=True)
    cnt = exp["inside"].sum(1)
    won = set(exp["obj"].tolist())
    assert cnt[255] and cnt[256] and cnt[257] and cnt[8191:].all() and cnt[:256].sum() >= 32
    assert any(o in won for o in (255, 256, 257)) and any(o in won for o in range(8191, 8200)) and any(0 <= o < 256 for o in won)
    res = eng.query_map(t, codes, pts, normals=True)
    st = eng.query_stats()
    plain = eng.query_map(t, codes, pts)
    for r, keys in ((res, ALL4), (plain, ALL4[:3])):
        _same({k: r[k][S] for k in keys}, exp, keys=keys)
        out = np.setdiff1d(np.arange(n), S)
        assert np.all(r["obj"][out] == -1) and np.all(np.isposinf(r["dist"][out])) and np.isfinite(r["bound"][out]).all()
    assert np.all(res["normal"][out] == 0)
    sample = rng.choice(out, 64, replace=False)
    rt, sc, ok = Q.invert(t)
    assert ok.all() and _bits_equal(res["bound"][sample], Q.candidates(rt, sc, pts[sample])[2])
    print("8200 objects: pass %d points, %d points, %d candidate rows in %d objects, stats %s" % (P, n, cnt.sum(), (cnt > 0).sum(), st))
    parity_log(case="map_scale_8200", pass_pts=P, points=n, candidate_rows=int(cnt.sum()), objects_with_rows=int((cnt > 0).sum()), **st)
    assert st["passes"] == 2 and st["rows"] == int(cnt.sum()) and eng.query_stats()["passes"] == 2


# ---- e. 65 540 hypotheses ----------------------------------------------------------------------------------------------------------------
N_HYP = 65540
_S24 = {}


def scene24(eng):
    """The three-object scene of tests/test_gpu_map_align.py cut to 8 points per object, and seven start poses that the hypotheses cycle
    through: T_true, four 5-degree offsets, one 30-degree offset, one 1e-4 off T_true."""
    if not _S24:
        fresh = not TA._SCENE
        base = dict(TA.scene(eng))
        if fresh:
            TA._SCENE.clear()           # built with THIS module's engine (its decode callback): not left behind for the other module
        rng = np.random.default_rng(65540)
        idx = np.concatenate([np.arange(0, 8), np.arange(100, 108), np.arange(200, 208)])
        c = base["centre"]
        poses = [T_TRUE] + [A.offset_pose(rng, T_TRUE, 5.0, 0.05, c) for _ in range(4)] + [A.offset_pose(rng, T_TRUE, 30.0, 0.3, c)]
        poses.append(A.offset_pose(np.random.default_rng(5), T_TRUE, 0.005, 1e-4, c))
        poses = np.stack(poses)
        _S24.update(t=base["t"], codes=base["codes"], map=base["map"], decode=TA._decoder(eng, base["codes"]), pts=base["pts"][idx], poses=poses,
                    hyp=poses[np.arange(N_HYP) % 7])
    return _S24


def _classes_are_uniform(res):
    """every hypothesis has the bytes of the first hypothesis of its class k mod 7, in every result array"""
    first = np.arange(N_HYP) % 7
    for key in TA.RESULT_KEYS:
        a = np.ascontiguousarray(res[key]).reshape(N_HYP, -1).view(np.uint8)
        bad = np.flatnonzero((a != a[first]).any(1))
        assert bad.size == 0, (key, bad[:8].tolist(), bad.size)


def test_65540_hypotheses_one_evaluation(eng):
    """65 535 mod 7 is 1: hypothesis k and hypothesis k - 65 535 start from different poses, so a wrong offset behind the grid split reads
    another pose's rows."""
    s = scene24(eng)
    assert N_HYP * 24 < 1 << 31 and 65535 % 7 == 1
    res = TA._align(eng, s, s["hyp"], iterations=1)
    st = eng.align_stats()
    for k in (0, 1, 65534, 65535, 65536, 65539):
        ev = TA._ref_eval(s, s["hyp"][k])
        TA._record_is(res, k, ev)
        assert np.array_equal(res["obj"][k], ev["obj"]) and TA._same32(res["dist"][k], ev["dist"]), k
        assert TA._same64(res["pose"][k], s["hyp"][k])
    _classes_are_uniform(res)
    size = np.bincount(np.arange(N_HYP) % 7, minlength=7)
    rows = [int(Q.candidates(s["map"].rt, s["map"].s, A.transform(T, s["pts"]))[1].sum()) for T in s["poses"]]
    assert st["rows"] == int((size * np.array(rows)).sum()) and st["evaluations"] == 1 and st["passes"] == -(-N_HYP * 24 // (1 << 17))
    assert len({res["cost"][k] for k in range(7)}) == 7               # the seven classes are seven different problems


def test_65540_hypotheses_with_ended_ones_on_both_sides_of_the_split(eng):
    """Two evaluations at the default tolerances: the hypotheses at T_true converge at their first evaluation
    (tests/test_gpu_map_align.py::test_an_ended_hypothesis_costs_no_rows), so the second evaluation runs with ended hypotheses on both
    sides of hypothesis 65 535.  Behind the split the live flag of hypothesis k is read through the offset pointer: hypothesis 65 535
    (class 1, live) sits where an unshifted pointer finds hypothesis 0 (class 0, ended)."""
    s = scene24(eng)
    res = TA._align(eng, s, s["hyp"], iterations=2)
    st = eng.align_stats()
    single = [TA._align(eng, s, s["poses"][c:c + 1], iterations=2, trace=True) for c in range(7)]
    assert single[0]["evaluations"][0] == 1 and single[0]["status"][0] == L.ALIGN_CONVERGED
    assert all(single[c]["evaluations"][0] == 2 for c in range(1, 7))
    for k in (0, 1, 65534, 65535, 65536, 65539):
        assert TA._bytes(res, k) == TA._bytes(single[k % 7]), k
    _classes_are_uniform(res)
    size = np.bincount(np.arange(N_HYP) % 7, minlength=7)
    rows = 0
    for c in range(7):
        for e in range(int(single[c]["evaluations"][0])):
            rows += int(size[c]) * int(Q.candidates(s["map"].rt, s["map"].s, A.transform(single[c]["trace"]["pose"][0, e], s["pts"]))[1].sum())
    assert st["rows"] == rows and st["evaluations"] == 2
