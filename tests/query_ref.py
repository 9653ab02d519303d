"""numpy restatement of dsp_slam_amd/csrc/query_math.h (the arithmetic of dsp_map_query): explicit float32 operations in the header's order.

fmaf: a float32 product is exact in float64, but rounding the float64 sum once more to float32 can differ from the single rounding of a real
fused multiply-add (a double-rounding tie).  fmaf32 below removes that case instead of hoping not to meet it: the sum's exact rounding error
is recovered with the TwoSum identity, and when the sum was inexact the float64 result is moved to its neighbour with an odd last bit
("rounding to odd"), after which the conversion to float32 rounds exactly as one rounding of the exact value would (53 >= 24 + 2 bits).  No
numpy.longdouble is needed.

The pose inversion is float64 in the header's written order, each output rounded once.
"""
import numpy as np

F32 = np.float32
TINY = F32(1e-20)
RIGID_TOL = float(F32(1e-4))


def fmaf32(a, b, c):
    """fl32(a * b + c) with ONE rounding, elementwise; a, b, c float32."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)          # exact
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                          # exact: p + c == s + err
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        # the exact value lies between s and its neighbour on err's side; that neighbour's last bit is odd
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def invert(t):
    """t: (n, 4, 4) float32 -> rt (n, 12) float32 [R_ow | t_ow] row-major 3 x 4, s (n,) float32, ok (n,) bool (False: the header refuses)."""
    t = np.asarray(t, F32).reshape(-1, 4, 4)
    a = t[:, :3, :3].astype(np.float64)
    tr = t[:, :3, 3].astype(np.float64)
    with np.errstate(all="ignore"):
        n = [(a[:, 0, c] * a[:, 0, c] + a[:, 1, c] * a[:, 1, c]) + a[:, 2, c] * a[:, 2, c] for c in range(3)]
        s2 = ((n[0] + n[1]) + n[2]) / 3.0
        s = np.sqrt(s2)
        rt = np.zeros((t.shape[0], 3, 4), np.float64)
        for i in range(3):
            row = [a[:, j, i] / s2 for j in range(3)]
            for j in range(3):
                rt[:, i, j] = row[j]
            rt[:, i, 3] = -((row[0] * tr[:, 0] + row[1] * tr[:, 1]) + row[2] * tr[:, 2])
        ok = np.isfinite(t).all((1, 2)) & (t[:, 3, 0] == 0) & (t[:, 3, 1] == 0) & (t[:, 3, 2] == 0) & (t[:, 3, 3] == 1) & (s2 > 0)
        for r in range(3):
            for c in range(3):
                d = np.zeros(t.shape[0])
                for k in range(3):
                    d = d + (a[:, k, r] / s) * (a[:, k, c] / s)
                ok &= np.abs(d - (1.0 if r == c else 0.0)) <= RIGID_TOL
        rt32, s32 = rt.reshape(-1, 12).astype(F32), s.astype(F32)
        ok &= np.isfinite(rt32).all(1) & np.isfinite(s32) & (s32 > 0)
    return rt32, s32, ok


def to_object(rt, pts):
    """rt (n_obj, 12), pts (n_pts, 3) -> p_obj (n_obj, n_pts, 3)."""
    rt = np.asarray(rt, F32).reshape(-1, 3, 4)
    p = np.asarray(pts, F32).reshape(-1, 3)
    x, y, z = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    out = np.zeros((rt.shape[0], p.shape[0], 3), F32)
    for i in range(3):
        r = rt[:, i, :, None]
        out[:, :, i] = fmaf32(r[:, 2], z, fmaf32(r[:, 1], y, fmaf32(r[:, 0], x, r[:, 3])))
    return out


def norm2(v):
    v = np.asarray(v, F32)
    with np.errstate(all="ignore"):
        return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def candidates(rt, scale, pts):
    """-> p_obj (n_obj, n_pts, 3), inside (n_obj, n_pts) bool, bound (n_pts,) float32."""
    scale = np.asarray(scale, F32)
    p_obj = to_object(rt, pts)
    n2 = norm2(p_obj)
    with np.errstate(all="ignore"):
        inside = n2 < F32(1)
        sb = (np.sqrt(n2) - F32(1)) * scale[:, None]
        bound = np.full(p_obj.shape[1], np.inf, F32)
        for o in range(p_obj.shape[0]):              # min_bound, ascending objects: fminf on numbers, a NaN candidate sticks
            v = sb[o]
            new = np.where(v < bound, v, np.where(np.isnan(v), v, bound))
            bound = np.where(inside[o], bound, new).astype(F32)
    return p_obj, inside, bound


def orderable(d):
    d = np.ascontiguousarray(d, F32)
    u = d.view(np.uint32)
    o = np.where(u & np.uint32(0x80000000), ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(d), np.uint32(0xffffffff), o)


def keys(d, obj):
    return (orderable(d).astype(np.uint64) << np.uint64(32)) | np.asarray(obj, np.int64).astype(np.uint32).astype(np.uint64)


def select(sdf, scale_of_row, obj_of_row, pt_of_row, n_pts):
    """-> obj (n_pts,) int32, dist (n_pts,) float32: the smallest key per point; a key whose high word is all ones is no winner."""
    with np.errstate(all="ignore"):
        d = np.asarray(sdf, F32) * np.asarray(scale_of_row, F32)
    k = keys(d, obj_of_row)
    best = np.full(n_pts, np.uint64(0xffffffffffffffff))
    np.minimum.at(best, np.asarray(pt_of_row, np.int64), k)
    hi = (best >> np.uint64(32)).astype(np.uint32)
    none = hi == np.uint32(0xffffffff)
    bits = np.where(hi & np.uint32(0x80000000), hi ^ np.uint32(0x80000000), ~hi).astype(np.uint32)
    dist = np.where(none, F32(np.inf), bits.view(F32)).astype(F32)
    obj = np.where(none, -1, (best & np.uint64(0xffffffff)).astype(np.int64)).astype(np.int32)
    return obj, dist


def normals(rt, g):
    """rt (n, 12) of each row's object, g (n, 3) object-frame gradients -> world unit normals (n, 3)."""
    rt = np.asarray(rt, F32).reshape(-1, 3, 4)
    g = np.asarray(g, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        g2 = norm2(g)
        u = np.zeros_like(g)
        for j in range(3):
            u[:, j] = fmaf32(rt[:, 2, j], g[:, 2], fmaf32(rt[:, 1, j], g[:, 1], rt[:, 0, j] * g[:, 0]))
        u2 = norm2(u)
        un = np.sqrt(u2)
        flat = (g2 < TINY) | (u2 == 0)
        n = u / un[:, None]
    return np.where(flat[:, None], F32(0), n).astype(F32)


def plan(cnt, budget):
    """How dsp_map_query cuts one pass into chunks, stated plainly: the list of all (object, candidate) pairs in order -- object 0's
    candidates 0, 1, ..., then object 1's -- cut every `budget` rows.  -> pairs (n_rows_total, 2) int64; chunk c holds
    pairs[c * budget:(c + 1) * budget], its row r is pairs[c * budget + r]."""
    cnt = np.asarray(cnt, np.int64)
    ob = np.repeat(np.arange(cnt.size, dtype=np.int64), cnt)
    first = np.cumsum(cnt) - cnt
    return np.stack([ob, np.arange(ob.size, dtype=np.int64) - first[ob]], 1)


TAU_DEC = 5e-6          # |fp32 decoder - float64 oracle|, the bound tests/test_gpu_decoders.py asserts


def expected64(dec, t_world_obj, codes, pts, ref):
    """The map query in plain float64, nothing restated from query_math.h: p_o = T^-1 p (numpy.linalg.inv of the float32 pose taken
    exactly), s = det(T[:3, :3]) ** (1 / 3), dist = s * sdf64(code, p_o) by the float64 oracle decoder `dec`, the normal R g / |g| with
    R = T[:3, :3] / s, the bound min over objects of (|p_o| - 1) s.  Only WHICH (object, point) pairs are decoded and which objects enter
    the bound is taken from the restatement `ref` (expected(...)): a point within rounding of a sphere's border is a candidate for one and
    not for the other, and that border is pinned bit for bit by tests/test_query_host.py.

    -> dict over the restatement's candidate rows (object-major, ascending points: ref["rows"]): obj, pt, d (s * sdf64), g (d sdf / d xyz,
    object frame), g_flip (the same with every ReLU within fp32 round-off of its kink on its other side; the round-off includes the
    point's own |p_o32 - p_o64|), n (world unit normal of g), delta (|p_o32 - p_o64|), tol (s (TAU_DEC + 2 |g| delta)); and per point
    bound, bound_tol (see tests/test_gpu_map_scale.py::test_large_map_against_float64)."""
    from oracle import dsp_oracle as O
    t = np.asarray(t_world_obj, F32).reshape(-1, 4, 4).astype(np.float64)
    p = np.asarray(pts, F32).reshape(-1, 3).astype(np.float64)
    inv = np.linalg.inv(t)
    s = np.cbrt(np.linalg.det(t[:, :3, :3]))
    ob, pt = ref["rows"]["obj"].astype(np.int64), ref["rows"]["pt"].astype(np.int64)
    p_o = np.einsum("nij,nj->ni", inv[ob, :3, :3], p[pt]) + inv[ob, :3, 3]
    dp = np.abs(ref["p_obj"][ob, pt].astype(np.float64) - p_o)
    delta = np.sqrt((dp * dp).sum(1))
    code = np.stack([np.asarray(c, F32)[:dec.code_len] for c in codes]).astype(np.float64)
    y, g, g_flip = O._decoder_fb64(dec, np.concatenate([code[ob], p_o], 1), True, dp)      # ONE call over all rows, each with its own code
    g, g_flip = g[:, -3:], g_flip[:, -3:]
    gn = np.sqrt((g * g).sum(1))
    rot = t[:, :3, :3] / s[:, None, None]
    n = np.einsum("nij,nj->ni", rot[ob], g) / gn[:, None]
    # the bound, dense: every object whose sphere the restatement puts the point outside of
    outside = ~ref["inside"]
    po_all = np.einsum("oij,pj->opi", inv[:, :3, :3], p) + inv[:, None, :3, 3]
    b_all = np.where(outside, (np.sqrt((po_all * po_all).sum(2)) - 1.0) * s[:, None], np.inf)
    eps32 = float(np.finfo(F32).eps)
    t_ow = np.sqrt((inv[:, :3, 3] ** 2).sum(1))
    tol_all = 4.0 * eps32 * (t_ow[:, None] + np.sqrt((p * p).sum(1))[None, :] / s[:, None]) * s[:, None]
    bound = b_all.min(0)
    # the fp32 minimum may sit at another object than the float64 one: any object within twice the largest tolerance of the minimum
    near = b_all <= bound[None, :] + 2.0 * tol_all.max(0)[None, :]
    bound_tol = np.where(near, tol_all, 0.0).max(0)
    return {"obj": ob, "pt": pt, "d": s[ob] * y, "g": g, "g_flip": g_flip, "n": n, "delta": delta, "scale": s,
            "tol": s[ob] * (TAU_DEC + 2.0 * gn * delta), "bound": bound, "bound_tol": bound_tol}


def random_rotations(rng, n):
    """uniform rotations (n, 3, 3) float64 from unit quaternions."""
    q = rng.normal(size=(n, 4))
    q /= np.sqrt((q * q).sum(1))[:, None]
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)


def sim3(rot, scale, trans):
    """(n, 4, 4) float32 object-to-world poses."""
    n = rot.shape[0]
    t = np.zeros((n, 4, 4))
    t[:, :3, :3] = rot * np.asarray(scale, np.float64).reshape(n, 1, 1)
    t[:, :3, 3] = trans
    t[:, 3, 3] = 1.0
    return t.astype(F32)


def expected(eng, t_world_obj, codes, pts, with_normals=False):
    """What dsp_map_query must return, composed from the entry points that existed before it: this file for transforms, containment and
    bounds, Engine.decode_sdf / Engine.sdf_jacobian per object at the reference's p_o, this file for selection and normals."""
    t = np.asarray(t_world_obj, F32).reshape(-1, 4, 4)
    pts = np.asarray(pts, F32).reshape(-1, 3)
    rt, s, ok = invert(t)
    assert ok.all()
    p_obj, inside, bound = candidates(rt, s, pts)
    sdf, sc, ob, pt, gr = [], [], [], [], []
    for o in range(t.shape[0]):
        idx = np.flatnonzero(inside[o])
        if idx.size == 0:
            continue
        if with_normals:
            v, g = eng.sdf_jacobian(codes[o], p_obj[o, idx])
            gr.append(g[:, -3:])
        else:
            v = eng.decode_sdf(codes[o], p_obj[o, idx])
        sdf.append(v); sc.append(np.full(idx.size, s[o], F32)); ob.append(np.full(idx.size, o, np.int32)); pt.append(idx)
    cat = lambda xs, dt, shape=(0,): np.concatenate(xs).astype(dt) if xs else np.zeros(shape, dt)
    sdf, sc, ob, pt = cat(sdf, F32), cat(sc, F32), cat(ob, np.int32), cat(pt, np.int32)
    obj, dist = select(sdf, sc, ob, pt, pts.shape[0])
    out = {"obj": obj, "dist": dist, "bound": bound, "inside": inside, "p_obj": p_obj, "rt": rt, "scale": s,
           "rows": {"sdf": sdf, "scale": sc, "obj": ob, "pt": pt}}
    if with_normals:
        g = cat(gr, F32, (0, 3)).reshape(-1, 3)
        nrm = np.zeros((pts.shape[0], 3), F32)
        win = obj[pt] == ob                           # the winning row of every point that has one (keys are unique per point and object)
        win &= keys(sdf * sc, ob) == keys(dist[pt], obj[pt])
        nrm[pt[win]] = normals(rt[ob[win]], g[win])
        out["normal"] = nrm
    return out
