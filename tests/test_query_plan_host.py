"""CPU-only: how dsp_map_query cuts a pass into chunks and tiles (dsp_debug_query_plan: the function the query itself calls, csrc/map_host.hip
query_plan_geometry and query_pass_pts) against the plain statement of the plan in tests/query_ref.py: the list of all (object, candidate)
pairs in order, cut every `budget` rows.

The cases are generated from fixed seeds; test_the_generator_reaches_every_corner asserts ON THE INPUTS that the corners the plan has are
among them, so that a change of the generator cannot lose one silently.
"""
import numpy as np
import pytest

import query_ref as Q
from dsp_slam_amd import _lib as L

E_ARG = -1
DEFAULT_BUDGET = 246723                 # 64 MiB of rows of 68 floats
BUDGETS = [1, 63, 64, 65, 70, 1000, DEFAULT_BUDGET, 1 << 24]
N_OBJ = [1, 5, 257, 600, 2000]
COUNTS = [1, 63, 64, 65, 300]
BIG = 131072
ZEROS = [(0.0, "none"), (0.2, "start"), (0.2, "middle"), (0.2, "end"), (0.4, "start"), (0.4, "middle"), (0.4, "end")]


def host_plan(cnt, budget, sizing_only=False):
    """dsp_debug_query_plan -> chunks (n, 4) {o0, nc, n_rows, nt}, base, tiles (nt_total, 4)"""
    lib = L.load()
    cnt = np.ascontiguousarray(cnt, np.int32)
    sizes = np.full(3, -7, np.int64)
    assert lib.dsp_debug_query_plan(cnt.size, L.ptr(cnt, L.c_i32p), budget, 0, L.ptr(sizes, L.c_i64p), None, None, None, None) == 0
    if sizing_only:
        return sizes
    chunks, base, tiles = np.full((sizes[0], 4), -7, np.int32), np.full(sizes[1], -7, np.int32), np.full((sizes[2], 4), -7, np.int32)
    again = np.zeros(3, np.int64)
    assert lib.dsp_debug_query_plan(cnt.size, L.ptr(cnt, L.c_i32p), budget, 0, L.ptr(again, L.c_i64p), L.ptr(chunks, L.c_i32p), L.ptr(base, L.c_i32p),
                                    L.ptr(tiles, L.c_i32p), None) == 0
    assert np.array_equal(again, sizes)
    return chunks, base, tiles


def pass_pts(n_obj):
    out = np.full(1, -7, np.int64)
    assert L.load().dsp_debug_query_plan(0, None, 0, n_obj, None, None, None, None, L.ptr(out, L.c_i64p)) == 0
    return int(out[0])


def count_vector(n_obj, frac, where, seed):
    """n_obj counts among COUNTS, one of them BIG (where there is room for it: early in the map, so that at the default budget the chunk
    behind it starts inside an object and goes on over the rest of the map), and round(frac n_obj) zeros: one run at the start or at the
    end, or -- "middle" -- half of them as one run in the middle and the other half scattered over the interior."""
    rng = np.random.default_rng(seed)
    cnt = rng.choice(COUNTS, n_obj).astype(np.int64)
    if n_obj >= 5:
        cnt[n_obj // 10 + 1] = BIG
    nz = int(round(frac * n_obj))
    if nz and where == "start":
        cnt[:nz] = 0
    elif nz and where == "end":
        cnt[n_obj - nz:] = 0
    elif nz:
        run = max(nz // 2, 1)
        cnt[n_obj // 2:n_obj // 2 + run] = 0
        if n_obj > 2 and nz > run:
            cnt[1 + rng.permutation(n_obj - 2)[:nz - run]] = 0
    return cnt


def cases(n_obj):
    for i, (frac, where) in enumerate(ZEROS):
        cnt = count_vector(n_obj, frac, where, 1000 * n_obj + i)
        for budget in BUDGETS:
            yield cnt, budget


def check_plan(cnt, budget):
    """every property of the plan of (cnt, budget), vectorised over its chunks"""
    cnt = np.asarray(cnt, np.int64)
    chunks, base, tiles = host_plan(cnt, budget)
    pairs = Q.plan(cnt, budget)
    R = pairs.shape[0]
    C = -(-R // budget)
    # n_rows <= budget, only the last chunk may be short, no chunk is empty; nc and nt are the lengths of what is returned
    assert chunks.shape[0] == C
    if C == 0:
        assert base.size == 0 and tiles.shape[0] == 0
        return chunks, base, tiles
    o0, nc, n_rows, nt = (chunks[:, k].astype(np.int64) for k in range(4))
    want_rows = np.full(C, budget, np.int64)
    want_rows[-1] = R - (C - 1) * budget
    assert np.array_equal(n_rows, want_rows) and n_rows.min() >= 1 and n_rows.max() <= budget
    assert nc.sum() == base.size and nt.sum() == tiles.shape[0] and nc.min() >= 1 and nt.min() >= 1
    assert o0.min() >= 0 and (o0 + nc).max() <= cnt.size
    boff, toff = np.cumsum(nc) - nc, np.cumsum(nt) - nt
    start = np.arange(C, dtype=np.int64) * budget                   # the chunk's first row in the list of all pairs
    # o0 is an object that has rows in the chunk: the object of the chunk's first row
    assert np.array_equal(o0, pairs[start, 0])
    # chunk row base[k] + j holds candidate j of object o0 + k: every pair of the list sits at its own row of its own chunk ...
    r = np.arange(R, dtype=np.int64)
    c_of = r // budget
    k = pairs[:, 0] - o0[c_of]
    assert k.min() >= 0 and np.all(k < nc[c_of])
    assert np.array_equal(base[boff[c_of] + k].astype(np.int64) + pairs[:, 1], r - start[c_of])
    # ... and nothing else maps into [0, n_rows): the rows that the chunk's objects would fill, clipped to the chunk, are n_rows in all
    c_of_b = np.repeat(np.arange(C), nc)
    ob_b = o0[c_of_b] + (np.arange(base.size) - boff[c_of_b])
    lo, hi = np.maximum(base.astype(np.int64), 0), np.minimum(base.astype(np.int64) + cnt[ob_b], n_rows[c_of_b])
    filled = np.zeros(C, np.int64)
    np.add.at(filled, c_of_b, np.maximum(hi - lo, 0))
    assert np.array_equal(filled, n_rows)
    # each tile covers 1 to 64 consecutive rows of ONE object; the tiles partition [0, n_rows) in order
    t_first, t_n, t_slot = (tiles[:, q].astype(np.int64) for q in range(3))
    c_of_t = np.repeat(np.arange(C), nt)
    assert t_n.min() >= 1 and t_n.max() <= 64 and not tiles[:, 3].any()
    is_first = np.zeros(tiles.shape[0], bool)
    is_first[toff] = True
    assert np.all(t_first[is_first] == 0)
    assert np.array_equal(t_first[1:][~is_first[1:]], (t_first + t_n)[:-1][~is_first[1:]])
    last = toff + nt - 1
    assert np.array_equal((t_first + t_n)[last], n_rows)
    g_first, g_last = start[c_of_t] + t_first, start[c_of_t] + t_first + t_n - 1
    assert np.array_equal(pairs[g_first, 0], pairs[g_last, 0])
    # slots count 0, 1, 2, ... over the chunk's objects that have rows; an object without rows has no slot
    new_obj = np.ones(R, bool)
    new_obj[1:] = pairs[1:, 0] != pairs[:-1, 0]
    new_obj[start] = True
    seen = np.cumsum(new_obj)
    slot_of_row = seen - seen[start[c_of]]
    assert np.array_equal(t_slot, slot_of_row[g_first])
    assert np.array_equal(t_slot[last] + 1, (seen[np.minimum(start + budget, R) - 1] - seen[start]) + 1)
    return chunks, base, tiles


@pytest.mark.parametrize("n_obj", N_OBJ)
def test_plan_is_the_list_of_pairs_cut_every_budget_rows(n_obj):
    n = 0
    for cnt, budget in cases(n_obj):
        check_plan(cnt, budget)
        n += 1
    assert n == len(ZEROS) * len(BUDGETS)


def _corners(cnt, budget):
    """(a budget ends exactly on an object's last candidate, a chunk starts inside an object and then spans more than 256 objects, a run
    of empty objects lies at a chunk border) -- from the inputs alone"""
    cnt = np.asarray(cnt, np.int64)
    R = int(cnt.sum())
    ends = np.cumsum(cnt)
    borders = np.arange(budget, R, budget, dtype=np.int64)          # a chunk ends and another begins
    at_end = np.isin(borders, ends[cnt > 0])
    exact = budget > 1 and bool(at_end.any())
    holds = lambda rows: np.searchsorted(ends, rows, side="right")  # the object that holds a row of the list
    wide = bool((~at_end & (holds(np.minimum(borders + budget, R) - 1) - holds(borders) > 256)).any())
    o = holds(borders - 1)                                          # the object of the last row in front of the border
    ok = at_end & (o + 2 < cnt.size)
    empty_run = bool((ok & (cnt[np.minimum(o + 1, cnt.size - 1)] == 0) & (cnt[np.minimum(o + 2, cnt.size - 1)] == 0)).any())
    return exact, wide, empty_run


def test_the_generator_reaches_every_corner():
    got = np.zeros(3, int)
    big = 0
    for n_obj in N_OBJ:
        for cnt, budget in cases(n_obj):
            got += np.array(_corners(cnt, budget), int)
            big += int((cnt == BIG).sum() == 1)
            assert set(np.unique(cnt).tolist()) <= set(COUNTS) | {0, BIG}
    assert got[0] >= 1, "no budget ends exactly on an object's last candidate"
    assert got[1] >= 1, "no chunk starts inside an object and then spans more than 256 objects"
    assert got[2] >= 1, "no run of empty objects at a chunk border"
    assert big >= 1
    # and the three by hand, so that each is also there in its smallest form
    for cnt, budget, want in (([64, 64, 1], 64, 0), ([1500] + [1] * 600, 1000, 1), ([70, 0, 0, 0, 5], 70, 2)):
        assert _corners(cnt, budget)[want]
        check_plan(cnt, budget)


def test_hand_built_plans():
    # the 5-object ragged map of tests/test_gpu_map_query.py, the empty object first: one chunk, slots skip nothing but object 0
    chunks, base, tiles = check_plan([0, 1, 63, 64, 65], DEFAULT_BUDGET)
    assert chunks.tolist() == [[1, 4, 193, 5]] and base.tolist() == [0, 1, 64, 128]
    assert tiles[:, :3].tolist() == [[0, 1, 0], [1, 63, 1], [64, 64, 2], [128, 64, 3], [192, 1, 3]]
    # an empty object in the MIDDLE of a chunk: slot != k from there on
    chunks, base, tiles = check_plan([2, 0, 3], 10)
    assert chunks.tolist() == [[0, 3, 5, 2]] and base.tolist() == [0, 2, 2] and tiles[:, :3].tolist() == [[0, 2, 0], [2, 3, 1]]
    # a chunk that starts inside an object: its base is negative
    chunks, base, tiles = check_plan([100, 3], 70)
    assert chunks.tolist() == [[0, 1, 70, 2], [0, 2, 33, 2]] and base.tolist() == [0, -70, 30]
    assert tiles[:, :3].tolist() == [[0, 64, 0], [64, 6, 0], [0, 30, 0], [30, 3, 1]]
    # nothing to do
    for cnt in ([], [0], [0, 0, 0]):
        assert host_plan(cnt, 64, sizing_only=True).tolist() == [0, 0, 0]
    # budget 0 is the default budget
    cnt = count_vector(600, 0.0, "none", 1)
    for a, b in zip(host_plan(cnt, 0), host_plan(cnt, DEFAULT_BUDGET)):
        assert np.array_equal(a, b)
    cnt = count_vector(2000, 0.0, "none", 1)
    assert host_plan(cnt, 0)[0].shape[0] == -(-int(cnt.sum()) // DEFAULT_BUDGET) > 1


def test_pass_points():
    for n in (1, 8191, 8192, 8193, 20000, 1 << 18):
        p = pass_pts(n)
        assert p % 64 == 0 and 64 <= p <= 1 << 17, (n, p)
        assert n * (p // 64) * 4 <= 64 << 20, (n, p)                 # the wave counts of a pass: n_obj x waves ints in 64 MiB
        assert p == 1 << 17 or n * (p // 64 + 1) * 4 > 64 << 20, (n, p)  # and not smaller than that requires
        if n <= 8192:
            assert p == 1 << 17, (n, p)
    assert pass_pts(8193) < 1 << 17 and pass_pts(8200) == 130944 and pass_pts(1 << 18) == 4096


def test_refusals():
    lib = L.load()
    cnt = np.array([3, -1, 2], np.int32)
    sizes, pp = np.zeros(3, np.int64), np.zeros(1, np.int64)
    s, c = L.ptr(sizes, L.c_i64p), L.ptr(cnt, L.c_i32p)
    assert lib.dsp_debug_query_plan(3, c, 64, 0, s, None, None, None, None) == E_ARG             # a negative count
    assert lib.dsp_debug_query_plan(1, c, 64, 0, s, None, None, None, None) == 0 and sizes.tolist() == [1, 1, 1]
    assert lib.dsp_debug_query_plan(1, None, 64, 0, s, None, None, None, None) == E_ARG
    assert lib.dsp_debug_query_plan(-1, c, 64, 0, s, None, None, None, None) == E_ARG
    assert lib.dsp_debug_query_plan(1, c, -1, 0, s, None, None, None, None) == E_ARG
    assert lib.dsp_debug_query_plan(1, c, (1 << 24) + 1, 0, s, None, None, None, None) == E_ARG
    assert lib.dsp_debug_query_plan((1 << 18) + 1, c, 64, 0, s, None, None, None, None) == E_ARG
    for bad in (0, -1, (1 << 18) + 1):
        assert lib.dsp_debug_query_plan(0, None, 0, bad, None, None, None, None, L.ptr(pp, L.c_i64p)) == E_ARG
    assert lib.dsp_debug_query_plan(0, None, 0, 0, None, None, None, None, None) == 0              # nothing asked, nothing refused
