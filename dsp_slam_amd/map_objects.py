"""MapObjects.txt -- the map dump DSP-SLAM writes at exit and `extract_map_objects.py` reads back.

Format (reference src/System_util.cc:123-146, extract_map_objects.py:46-63), three lines per object:
    <object id>
    <3x4 Sim(3) object->world pose, 12 numbers, row-major, 9 significant digits>
    <shape code, 64 numbers>
"""
import numpy as np


def read_map_objects(path):
    """-> list of dict(id=int, pose=(4,4) float64 Sim(3) T_world_obj, code=(C,) float32)."""
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip() != ""]
    if len(lines) % 3:
        raise ValueError("%s: expected 3 lines per object, got %d lines" % (path, len(lines)))
    out = []
    for i in range(len(lines) // 3):
        obj_id = int(lines[3 * i].strip())
        pose = np.array([float(x) for x in lines[3 * i + 1].split()], np.float64)
        if pose.size != 12:
            raise ValueError("%s: object %d pose has %d numbers" % (path, obj_id, pose.size))
        pose = np.concatenate([pose.reshape(3, 4), [[0., 0., 0., 1.]]], 0)
        code = np.array([float(x) for x in lines[3 * i + 2].split()], np.float32)
        out.append(dict(id=obj_id, pose=pose, code=code))
    return out


def write_map_objects(path, objects):
    """objects: iterable of dict(id, pose (4,4) or (3,4), code).  Laid out after System::SaveMapCurrentFrame (src/System_util.cc:123-146):
    `fixed`, setprecision(9); the pose as twelve scalars separated by single spaces; the code right-aligned to the width of the widest
    coefficient, as Eigen's default IOFormat streams a row vector (values separated by one OR MORE spaces -- the reason the reference's
    reader skips empty items, extract_map_objects.py:59-61).
    PARITY: reader-level only.  The reference's writer is C++ / Eigen and cannot be run in this image, so the exact bytes it emits are
    not pinned; what is pinned is that the reference's own parse loop (extract_map_objects.py:46-63, run through `runpy` in
    tests/test_gpu_map_tools.py) reads these files back to the values written."""
    with open(path, "w") as f:
        for o in sorted(objects, key=lambda x: x["id"]):
            f.write("%d\n" % int(o["id"]))
            p = np.asarray(o["pose"], np.float32)[:3, :4].reshape(-1)        # Eigen::Matrix4f / Vector<float,64>: float32 values
            f.write(" ".join("%.9f" % float(v) for v in p) + "\n")
            items = ["%.9f" % float(v) for v in np.asarray(o["code"], np.float32).reshape(-1)]
            width = max(len(x) for x in items) if items else 0
            f.write(" ".join(x.rjust(width) for x in items) + "\n")


def query_points(engine, objects, pts_world, normals=False):
    """Engine.query_map on the list read_map_objects returns: which object of the map every world point belongs to, its signed distance to that
    object's surface (world units) and -- normals=True -- the surface's outward normal there.  The result dict of Engine.query_map (obj, dist,
    bound, normal) plus `id`: the map's object id per point, -1 where obj is -1."""
    objects = list(objects)
    poses = np.stack([np.asarray(o["pose"], np.float64) for o in objects]) if objects else np.zeros((0, 4, 4))
    res = engine.query_map(poses, [o["code"] for o in objects], pts_world, normals=normals)
    return with_ids(res, [o["id"] for o in objects])


def localise(engine, objects, pts_sensor, t_world_sensor0, weights=None, trace=False, **params):
    """Engine.align_to_map on the list read_map_objects returns: the sensor-to-world pose that puts the sensor-frame points on the map's
    surfaces, one Gauss-Newton run per initial pose of t_world_sensor0.  The result dict of Engine.align_to_map with per-point `obj` /
    `dist` at every returned pose, plus `id`: the map's object id per hypothesis and point, -1 where obj is -1."""
    objects = list(objects)
    poses = np.stack([np.asarray(o["pose"], np.float64) for o in objects]) if objects else np.zeros((0, 4, 4))
    res = engine.align_to_map(poses, [o["code"] for o in objects], pts_sensor, t_world_sensor0, weights=weights, trace=trace, per_point=True, **params)
    return with_ids(res, [o["id"] for o in objects])


def cast_rays(engine, objects, origins, dirs, normals=False, **params):
    """Engine.cast_rays on the list read_map_objects returns: the first object surface along every world ray.  The result dict of
    Engine.cast_rays (obj, t, dist, status, normal) plus `id`: the map's object id per ray, -1 where obj is -1."""
    objects = list(objects)
    poses = np.stack([np.asarray(o["pose"], np.float64) for o in objects]) if objects else np.zeros((0, 4, 4))
    res = engine.cast_rays(poses, [o["code"] for o in objects], origins, dirs, normals=normals, **params)
    return with_ids(res, [o["id"] for o in objects])


def pixel_rays(K, t_world_cam, width, height):
    """One world ray per pixel centre, row-major ((height * width, 3) float32 origins and directions) and cos ((height * width,) float64,
    the cosine between each ray and the optical axis).  Pixel convention: integer pixel coordinates ARE the pixel centres (OpenCV's): the
    pixel in column j and row i looks along K^-1 (j, i, 1) = ((j - cx) / fx, (i - cy) / fy, 1) in the camera frame (x right, y down, z
    forward).  K: (3, 3) or (fx, fy, cx, cy); t_world_cam: (4, 4) rigid camera-to-world."""
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else K.reshape(4)
    T = np.asarray(t_world_cam, np.float64).reshape(4, 4)
    j, i = np.meshgrid(np.arange(int(width), dtype=np.float64), np.arange(int(height), dtype=np.float64))
    d_cam = np.stack([(j - cx) / fx, (i - cy) / fy, np.ones_like(j)], -1).reshape(-1, 3)
    dirs = (d_cam @ T[:3, :3].T).astype(np.float32)
    origins = np.broadcast_to(T[:3, 3].astype(np.float32), dirs.shape).copy()
    d64 = dirs.astype(np.float64)
    u = d64 / np.sqrt((d64 * d64).sum(1))[:, None]
    return origins, dirs, u @ T[:3, 2]                  # (R_cw u)_z = u . (third column of R_wc)


def render(engine, objects, K, t_world_cam, width, height, normals=False, **params):
    """What the map looks like from a pinhole camera: one ray per pixel centre (pixel_rays states the convention) through cast_rays.  A dict
    of (height, width) images: `depth` (float32 z-depth t * (R_cw u)_z, +inf where nothing is hit), `id` (int64 map object id, -1 where
    nothing is hit), `obj` (int32 index into `objects`), `status` (int32), `t`, `dist`, and with normals=True `normal` ((height, width, 3)
    world unit normals, else None)."""
    origins, dirs, cos = pixel_rays(K, t_world_cam, width, height)
    res = cast_rays(engine, objects, origins, dirs, normals=normals, **params)
    shape = (int(height), int(width))
    with np.errstate(invalid="ignore"):
        depth = np.where(res["obj"] >= 0, res["t"].astype(np.float64) * cos, np.inf).astype(np.float32)
    out = {"depth": depth.reshape(shape), "id": res["id"].reshape(shape), "obj": res["obj"].reshape(shape), "status": res["status"].reshape(shape),
           "t": res["t"].reshape(shape), "dist": res["dist"].reshape(shape), "normal": None}
    if normals:
        out["normal"] = res["normal"].reshape(shape + (3,))
    return out


def localise_rays(engine, objects, pts_sensor, t_world_sensor0, origins=None, weights=None, trace=False, **params):
    """Engine.align_rays_to_map on the list read_map_objects returns: the sensor-to-world pose at which the map, cast along the sensor's
    rays, shows the measured depths.  The result dict of Engine.align_rays_to_map with the per-ray outputs at every returned pose, plus
    `id`: the map's object id per hypothesis and ray, -1 where the ray is unmatched.  params: max_gap, raycast={...} and the fields of
    Engine.align_params."""
    objects = list(objects)
    poses = np.stack([np.asarray(o["pose"], np.float64) for o in objects]) if objects else np.zeros((0, 4, 4))
    res = engine.align_rays_to_map(poses, [o["code"] for o in objects], pts_sensor, t_world_sensor0, origins=origins, weights=weights, trace=trace,
                                   per_ray=True, **params)
    return with_ids(res, [o["id"] for o in objects])


def backproject_depth(depth, K):
    """The camera-frame points of a z-depth image by the pixel_rays convention: pixel (column j, row i) with depth z is
    z * ((j - cx) / fx, (i - cy) / fy, 1).  -> points (n, 3) float32 and their flat pixel indices (n,), row-major; pixels whose depth is
    not finite or not positive are skipped."""
    depth = np.asarray(depth, np.float64)
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else K.reshape(4)
    height, width = depth.shape
    j, i = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    z = depth.reshape(-1)
    with np.errstate(invalid="ignore"):
        keep = np.flatnonzero(np.isfinite(z) & (z > 0))
    d_cam = np.stack([(j - cx) / fx, (i - cy) / fy, np.ones_like(j)], -1).reshape(-1, 3)
    return (d_cam[keep] * z[keep, None]).astype(np.float32), keep


def localise_depth(engine, objects, depth, K, t_world_cam0, weights=None, trace=False, **params):
    """localise_rays on a z-depth image (height, width) of a pinhole camera: every pixel with a finite positive depth is one ray from the
    camera centre (backproject_depth; the convention of pixel_rays and render, so render(...)["depth"] fed back at the rendering pose
    costs about nothing there).  weights: None or an image.  The result of localise_rays plus `pixel`: the flat row-major pixel index of
    every ray."""
    pts, keep = backproject_depth(depth, K)
    w = None if weights is None else np.asarray(weights, np.float32).reshape(-1)[keep]
    res = localise_rays(engine, objects, pts, t_world_cam0, weights=w, trace=trace, **params)
    res["pixel"] = keep
    return res


def refine_poses(engine, objects, pts_world, origins_world, weights=None, only=None, trace=False, **params):
    """Engine.align_objects_to_rays on the list read_map_objects returns: the sensor poses are known, the OBJECTS are moved to where the
    world-frame depth rays (measured end points and ray origins, the rays of several frames concatenated) say they are.  only: None (every
    object) or the ids to refine; the others keep their pose and still occlude.  -> (result, objects): the result dict of
    Engine.align_objects_to_rays indexed like `objects`, with the per-ray outputs at the returned map and `id` (the map's object id per
    ray, -1 where the ray is unmatched), and a new object list with the returned poses.  params: max_gap, raycast={...} and the fields of
    Engine.align_params."""
    objects = list(objects)
    poses = np.stack([np.asarray(o["pose"], np.float64) for o in objects]) if objects else np.zeros((0, 4, 4))
    refine = None
    if only is not None:
        ids = [int(o["id"]) for o in objects]
        missing = [int(i) for i in only if int(i) not in ids]
        if missing:
            raise ValueError("refine_poses: no object with id %s in the map" % missing)
        refine = np.array([i in {int(x) for x in only} for i in ids], np.uint8)
    res = engine.align_objects_to_rays(poses, [o["code"] for o in objects], pts_world, origins_world, weights=weights, refine=refine, trace=trace,
                                       per_ray=True, **params)
    moved = [dict(o, pose=np.asarray(t, np.float64).copy()) for o, t in zip(objects, res["t_world_obj"])]
    return with_ids(res, [o["id"] for o in objects]), moved


def _depth_rays(depth, K, t_world_cam, weights):
    """z-depth images of pinhole cameras at known poses -> world-frame rays: (pts, origins, weights or None, pixel, frame)"""
    def images(x):
        return list(x) if isinstance(x, (list, tuple)) or np.asarray(x).ndim == 3 else [x]
    frames, cams = images(depth), images(t_world_cam)
    wimgs = [None] * len(frames) if weights is None else images(weights)
    if len(cams) != len(frames) or len(wimgs) != len(frames):
        raise ValueError("one pose (and one weight image) per depth image")
    pts, org, w, pixel, frame = [], [], [], [], []
    for f, (img, cam, wimg) in enumerate(zip(frames, cams, wimgs)):
        p_cam, keep = backproject_depth(img, K)
        T = np.asarray(cam, np.float64).reshape(4, 4)
        pts.append((p_cam.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32))
        org.append(np.broadcast_to(T[:3, 3].astype(np.float32), p_cam.shape).copy())
        pixel.append(keep)
        frame.append(np.full(keep.size, f, np.int64))
        if wimg is not None:
            w.append(np.asarray(wimg, np.float32).reshape(-1)[keep])
    return np.concatenate(pts), np.concatenate(org), np.concatenate(w) if w else None, np.concatenate(pixel), np.concatenate(frame)


def refine_poses_depth(engine, objects, depth, K, t_world_cam, weights=None, only=None, trace=False, **params):
    """refine_poses on z-depth images of pinhole cameras at KNOWN poses: one image (height, width) with its (4, 4) camera-to-world pose, or
    lists of both.  Every pixel with a finite positive depth is one ray from its camera's centre (backproject_depth: the convention of
    pixel_rays and render).  weights: None, or an image per frame.  The result of refine_poses plus `pixel` (the flat row-major pixel index
    of every ray) and `frame` (the index of its image)."""
    pts, org, w, pixel, frame = _depth_rays(depth, K, t_world_cam, weights)
    res, moved = refine_poses(engine, objects, pts, org, weights=w, only=only, trace=trace, **params)
    res["pixel"], res["frame"] = pixel, frame
    return res, moved


def refine_shapes(engine, objects, pts_world, origins_world, weights=None, only=None, trace=False, **params):
    """Engine.align_shapes_to_rays on the list read_map_objects returns: the sensor poses are known, the objects' SHAPE CODES -- and with
    unknowns="pose+code" their poses -- are refitted to the world-frame depth rays, inside the map (occlusion, a ray charged only to the
    object it sees).  Arguments and result as refine_poses; the new object list carries the returned codes and poses.  params: unknowns,
    code_reg, code_anchor, code_tol, max_gap, raycast={...} and the fields of Engine.align_params."""
    objects = list(objects)
    poses = np.stack([np.asarray(o["pose"], np.float64) for o in objects]) if objects else np.zeros((0, 4, 4))
    refine = None
    if only is not None:
        ids = [int(o["id"]) for o in objects]
        missing = [int(i) for i in only if int(i) not in ids]
        if missing:
            raise ValueError("refine_shapes: no object with id %s in the map" % missing)
        refine = np.array([i in {int(x) for x in only} for i in ids], np.uint8)
    res = engine.align_shapes_to_rays(poses, [o["code"] for o in objects], pts_world, origins_world, weights=weights, refine=refine, trace=trace,
                                      per_ray=True, **params)
    new = [dict(o, pose=np.asarray(t, np.float64).copy(), code=np.asarray(c, np.float32)[:np.asarray(o["code"]).reshape(-1).shape[0]].copy())
           for o, t, c in zip(objects, res["t_world_obj"], res["codes"])]
    return with_ids(res, [o["id"] for o in objects]), new


def refine_shapes_depth(engine, objects, depth, K, t_world_cam, weights=None, only=None, trace=False, **params):
    """refine_shapes on z-depth images of pinhole cameras at KNOWN poses, as refine_poses_depth: the result of refine_shapes plus `pixel`
    and `frame`."""
    pts, org, w, pixel, frame = _depth_rays(depth, K, t_world_cam, weights)
    res, new = refine_shapes(engine, objects, pts, org, weights=w, only=only, trace=trace, **params)
    res["pixel"], res["frame"] = pixel, frame
    return res, new


def with_ids(result, ids):
    """result (an Engine.query_map dict) with `id` added: ids[obj] per point, -1 where obj is -1."""
    out = dict(result)
    obj = np.asarray(result["obj"], np.int64)
    table = np.asarray(list(ids) + [-1], np.int64)          # obj == -1 reads the last entry
    out["id"] = table[obj]
    return out


def associate(result, max_dist):
    """Per object id of a query_points result, the indices (ascending) of the points it won with dist <= max_dist: {id: int64 array}.  Objects
    that won no such point are absent."""
    ids = np.asarray(result["id"], np.int64)
    keep = np.flatnonzero((np.asarray(result["obj"]) >= 0) & (np.asarray(result["dist"]) <= max_dist))
    return {int(i): keep[ids[keep] == i] for i in np.unique(ids[keep])}
