"""numpy restatement of the opening comment of dsp_slam_amd/csrc/raycast_math.h (the arithmetic of dsp_map_raycast): explicit float32 operations
in the comment's order, fmaf restated as tests/query_ref.py does (fmaf32: one rounding).  The geometry part (rays, segments, step) runs on
the CPU; expected() marches the pairs round by round and decodes through Engine.decode_sdf / Engine.sdf_jacobian, entry points that existed
before dsp_map_raycast, at the restatement's own object-frame samples.
"""
import numpy as np

import query_ref as Q

F32 = np.float32
STEP_HIT, STEP_MISS, STEP_ADVANCE, STEP_EXIT = 0, 1, 2, 3
MISS, HIT, UNDECIDED = 0, 1, 2
DEFAULTS = dict(t_min=0.0, t_max=np.inf, eps=1e-3, relax=1.0, max_steps=64)
DEFAULT_BUDGET = (64 << 20) // (68 * 4)         # the map query's chunk budget in rows
NONE32 = np.uint32(0xffffffff)
NONE64 = np.uint64(0xffffffffffffffff)


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in p, k
        p[k] = v
    return p


def check(p):
    """True: the params are accepted."""
    t_min, t_max, eps, relax = F32(p["t_min"]), F32(p["t_max"]), F32(p["eps"]), F32(p["relax"])
    return bool(t_min >= 0 and np.isfinite(t_min) and t_max > t_min and eps > 0 and np.isfinite(eps) and relax > 0 and relax <= 1
                and 1 <= int(p["max_steps"]) <= 4096)


def rays(origins, dirs):
    """-> u (n, 3) float32 unit directions (garbage for void rays), void (n,) bool."""
    o = np.asarray(origins, F32).reshape(-1, 3)
    d = np.asarray(dirs, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        n2 = Q.norm2(d)
        length = np.sqrt(n2)
        u = (d / length[:, None]).astype(F32)
        void = ~np.isfinite(o).all(1) | ~np.isfinite(d).all(1) | ~(n2 > 0) | ~np.isfinite(n2)
    return u, void


def segments(rt, s_sel, origins, u, void, t_min, t_max):
    """-> dict: exists (n_obj, n) bool, t0, t1 (n_obj, n), o_o, d_o (n_obj, n, 3), all float32."""
    rt3 = np.asarray(rt, F32).reshape(-1, 3, 4)
    o = np.asarray(origins, F32).reshape(-1, 3)
    t_min, t_max = F32(t_min), F32(t_max)
    with np.errstate(all="ignore"):
        o_o = Q.to_object(rt, o)
        d_o = np.zeros_like(o_o)
        for i in range(3):
            r = rt3[:, i, :, None]
            d_o[:, :, i] = Q.fmaf32(r[:, 2], u[None, :, 2], Q.fmaf32(r[:, 1], u[None, :, 1], r[:, 0] * u[None, :, 0]))
        a = Q.norm2(d_o)
        b = (o_o[..., 0] * d_o[..., 0] + o_o[..., 1] * d_o[..., 1]) + o_o[..., 2] * d_o[..., 2]
        c = Q.norm2(o_o) - F32(1)
        disc = Q.fmaf32(b, b, -(a * c))
        q = np.sqrt(disc)
        t_in = ((-b) - q) / a
        t_out = (q - b) / a
        exists = (disc > 0) & (t_out > t_min) & (t_in < t_max) & ~np.isnan(np.asarray(s_sel, F32))[:, None] & ~void[None, :]
        t0 = np.where(t_in > t_min, t_in, t_min).astype(F32)
        t1 = np.where(t_out < t_max, t_out, t_max).astype(F32)
    return {"exists": exists, "t0": t0, "t1": t1, "o_o": o_o, "d_o": d_o}


def sample(o_o, d_o, t):
    return Q.fmaf32(np.asarray(t, F32)[:, None], d_o, o_o)


def step(t, t1, sdf, s, eps, relax):
    """-> decision (int32), dist, t_next (float32)."""
    t, t1, sdf, s = [np.asarray(x, F32) for x in (t, t1, sdf, s)]
    with np.errstate(all="ignore"):
        d = (sdf * s).astype(F32)
        tn = Q.fmaf32(F32(relax), d, t)
        dec = np.where(np.isnan(d), STEP_MISS, np.where(d <= F32(eps), STEP_HIT, np.where(tn > t1, STEP_EXIT, STEP_ADVANCE))).astype(np.int32)
    return dec, d, np.where(dec >= STEP_ADVANCE, tn, t).astype(F32)


def from_orderable(hi):
    hi = np.asarray(hi, np.uint32)
    return np.where(hi & np.uint32(0x80000000), hi ^ np.uint32(0x80000000), ~hi).astype(np.uint32).view(F32)


def geometry(t_world_obj, code_finite, origins, dirs, p):
    """The CPU part: the table, the rays and every pair's segment.  code_finite: (n_obj,) bool."""
    t = np.asarray(t_world_obj, F32).reshape(-1, 4, 4)
    rt, s, ok = Q.invert(t)
    assert ok.all()
    s_sel = np.where(np.asarray(code_finite, bool), s, F32(np.nan)).astype(F32)
    u, void = rays(origins, dirs)
    seg = segments(rt, s_sel, origins, u, void, p["t_min"], p["t_max"])
    seg.update(rt=rt, scale=s, u=u, void=void)
    return seg


def expected(eng, t_world_obj, codes, origins, dirs, p=None, with_normals=False, budget=None):
    """What dsp_map_raycast must return (obj, t, dist, status, normal), its stats, the geometry and per ray `exhausted_at`: the orderable bits of
    the smallest parameter among its exhausted pairs, all ones for none.  budget: pairs per pass."""
    p = params(**(p or {}))
    assert check(p)
    budget = int(budget or DEFAULT_BUDGET)
    n = np.asarray(origins).reshape(-1, 3).shape[0]
    code_finite = np.array([np.isfinite(np.asarray(c, F32)[:eng.code_len]).all() for c in codes], bool)
    g = geometry(t_world_obj, code_finite, origins, dirs, p)
    n_obj = g["exists"].shape[0]
    ob_all = np.concatenate([np.full(int(g["exists"][o].sum()), o, np.int64) for o in range(n_obj)] + [np.zeros(0, np.int64)])
    ray_all = np.concatenate([np.flatnonzero(g["exists"][o]) for o in range(n_obj)] + [np.zeros(0, np.int64)])
    best = np.full(n, NONE64)
    exh = np.full(n, NONE32)
    dist_out = np.full(n, np.inf, F32)
    st = {"pairs": int(ob_all.size), "rows": 0, "tiles": 0, "rounds": 0, "passes": 0, "exhausted": 0, "retired": 0,
          "pairs_per_ray": g["exists"].sum(0), "rows_per_round": []}
    for first in range(0, ob_all.size, budget):
        ob, ray = ob_all[first:first + budget], ray_all[first:first + budget]
        st["passes"] += 1
        tcur, t1 = g["t0"][ob, ray].copy(), g["t1"][ob, ray]
        state = np.zeros(ob.size, np.int32)
        dist_p = np.zeros(ob.size, F32)
        for _ in range(int(p["max_steps"])):
            hi = (best[ray] >> np.uint64(32)).astype(np.uint32)                 # the keys as the previous round left them
            retire = (state == 0) & (hi != NONE32) & (tcur > from_orderable(hi))
            state[retire] = 2
            st["retired"] += int(retire.sum())
            live = np.flatnonzero(state == 0)
            if live.size == 0:
                break
            st["rows"] += int(live.size)
            st["rounds"] += 1
            st["rows_per_round"].append(int(live.size))
            sdf = np.zeros(live.size, F32)
            for o in np.unique(ob[live]):
                m = ob[live] == o
                idx = live[m]
                st["tiles"] += -(-int(idx.size) // 64)
                sdf[m] = eng.decode_sdf(codes[o], sample(g["o_o"][o, ray[idx]], g["d_o"][o, ray[idx]], tcur[idx]))
            dec, d, tn = step(tcur[live], t1[live], sdf, g["scale"][ob[live]], p["eps"], p["relax"])
            hit = live[dec == STEP_HIT]
            state[hit] = 1
            dist_p[hit] = d[dec == STEP_HIT]
            np.minimum.at(best, ray[hit], Q.keys(tcur[hit], ob[hit]))
            state[live[(dec == STEP_MISS) | (dec == STEP_EXIT)]] = 2
            adv = dec == STEP_ADVANCE
            tcur[live[adv]] = tn[adv]
        ex = state == 0
        st["exhausted"] += int(ex.sum())
        np.minimum.at(exh, ray[ex], Q.orderable(tcur[ex]))
        won = np.flatnonzero(state == 1)
        won = won[Q.keys(tcur[won], ob[won]) == best[ray[won]]]
        dist_out[ray[won]] = dist_p[won]
    hi = (best >> np.uint64(32)).astype(np.uint32)
    none = hi == NONE32
    obj = np.where(none, -1, (best & np.uint64(0xffffffff)).astype(np.int64)).astype(np.int32)
    t_hit = np.where(none, F32(np.inf), from_orderable(hi)).astype(F32)
    status = np.where(none, np.where(exh != NONE32, UNDECIDED, MISS), np.where(exh < hi, UNDECIDED, HIT)).astype(np.int32)
    out = {"obj": obj, "t": t_hit, "dist": dist_out, "status": status, "normal": None, "stats": st, "geometry": g, "exhausted_at": exh}
    if with_normals:
        nrm = np.zeros((n, 3), F32)
        for o in range(n_obj):
            idx = np.flatnonzero(obj == o)
            if idx.size:
                _, grad = eng.sdf_jacobian(codes[o], sample(g["o_o"][o, idx], g["d_o"][o, idx], t_hit[idx]))
                nrm[idx] = Q.normals(np.repeat(g["rt"][o:o + 1], idx.size, 0), grad[:, -3:])
        out["normal"] = nrm
    return out


def stats_of(st):
    return {k: st[k] for k in ("pairs", "rows", "tiles", "rounds", "passes", "exhausted")}
