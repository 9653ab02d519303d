"""Reading an observation report (Batch.report(), include/dsp_gn.h: dsp_batch_report): which points, rays and views disagree with the
state a run returned.  numpy only; no threshold is chosen for the caller.

A report's arrays are concatenated in MEMBER order (a member is an object, or a view of a multi-view batch); pts_off / ray_off cut them
per member and view_off groups the members per object.
"""
import numpy as np


def _members(report):
    return len(report["pts_off"]) - 1


_PER_POINT = ("pt_sdf", "pt_flags", "pt_alive")
_PER_RAY = ("ray_depth", "ray_hit", "ray_residual", "ray_counts")
_PER_MEMBER = ("M", "V", "m", "K", "sum_s", "sum_r", "status")


def object_rows(report, obj):
    """The rows of ONE object cut out of a report, as a report of its own (offsets rebased to 0): all its views for a multi-view batch,
    its one member otherwise.  What Optimizer results carry as `observations` and tools/reoptimise_map.py writes per object id."""
    vo = np.asarray(report["view_off"], np.int64)
    m0, m1 = int(vo[obj]), int(vo[obj + 1])
    po, ro, do = (np.asarray(report[k], np.int64) for k in ("pts_off", "ray_off", "depth_off"))
    out = {k: np.array(report[k][po[m0]:po[m1]]) for k in _PER_POINT}
    out.update({k: np.array(report[k][ro[m0]:ro[m1]]) for k in _PER_RAY})
    out.update({k: np.array(report[k][m0:m1]) for k in _PER_MEMBER})
    out.update(pts_off=po[m0:m1 + 1] - po[m0], ray_off=ro[m0:m1 + 1] - ro[m0], depth_off=do[m0:m1 + 1] - do[m0],
               view_off=np.array([0, m1 - m0], np.int64))
    return out


def point_outliers(report, tol):
    """Per member, a boolean mask over its surface points: |sdf| > tol, or the point is dead (dropped by the pose-only inlier filter, or
    its member was not evaluated: NaN).  The replacement of a box test on the map points: the signed distance to the fitted surface is
    what the optimiser itself minimised."""
    sdf = np.asarray(report["pt_sdf"])
    alive = np.asarray(report["pt_alive"], bool)
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(sdf) <= float(tol)) | ~alive
    off = np.asarray(report["pts_off"], np.int64)
    return [bad[off[i]:off[i + 1]] for i in range(_members(report))]


def view_scores(report, prm):
    """Per member (view), score = k2 sum_s / M + k1 sum_r / K -- a term whose count is 0 contributes nothing; a member that was not
    evaluated scores NaN -- and ratio = score / the median score of the views of ITS object (NaN-aware; 0 / 0 = NaN).
    prm: anything with k1 and k2 (engine.gn_params, a dict).  Returns dict(score, ratio) of float64 (n_members,)."""
    k1 = float(prm["k1"] if isinstance(prm, dict) else prm.k1)
    k2 = float(prm["k2"] if isinstance(prm, dict) else prm.k2)
    M, K = np.asarray(report["M"], np.float64), np.asarray(report["K"], np.float64)
    ss, sr = np.asarray(report["sum_s"], np.float64), np.asarray(report["sum_r"], np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        score = k2 * np.where(M > 0, ss / np.where(M > 0, M, 1.0), np.where(np.isnan(ss), np.nan, 0.0)) + \
                k1 * np.where(K > 0, sr / np.where(K > 0, K, 1.0), np.where(np.isnan(sr), np.nan, 0.0))
        ratio = np.full_like(score, np.nan)
        vo = np.asarray(report["view_off"], np.int64)
        for i in range(len(vo) - 1):
            s = score[vo[i]:vo[i + 1]]
            if s.size and not np.all(np.isnan(s)):
                ratio[vo[i]:vo[i + 1]] = s / np.nanmedian(s)
    return dict(score=score, ratio=ratio)


def silhouette_disagreement(report, n_fg=None):
    """Per member: fg_miss = the share of its foreground rays with hit < 0.5 (the mask says object, the shape says background) and
    bg_hit = the share of its background rays with hit > 0.5.  n_fg: foreground rays per member (default: the report's depth_off).
    NaN where a member has no ray of that kind or was not evaluated.  Returns dict(fg_miss, bg_hit) of float64 (n_members,)."""
    n = _members(report)
    ro = np.asarray(report["ray_off"], np.int64)
    if n_fg is None:
        n_fg = np.diff(np.asarray(report["depth_off"], np.int64))
    n_fg = np.broadcast_to(np.asarray(n_fg, np.int64), (n,))
    hit = np.asarray(report["ray_hit"], np.float64)
    fg_miss, bg_hit = np.full(n, np.nan), np.full(n, np.nan)
    for i in range(n):
        h = hit[ro[i]:ro[i + 1]]
        if h.size == 0 or np.all(np.isnan(h)):
            continue
        fg, bg = h[:n_fg[i]], h[n_fg[i]:]
        if fg.size:
            fg_miss[i] = float(np.mean(fg < 0.5))
        if bg.size:
            bg_hit[i] = float(np.mean(bg > 0.5))
    return dict(fg_miss=fg_miss, bg_hit=bg_hit)


def reject(report, pt_sdf_max, ray_res_max):
    """The report turned into per-observation weights (Batch.set_observation_weights): (pt_w, ray_w) of float32, concatenated in member
    order like the report.  pt_w is 0 where |pt_sdf| > pt_sdf_max or the point is not alive (dropped by the pose-only inlier filter, or its
    member was not evaluated), ray_w is 0 where |ray_residual| > ray_res_max; 1 elsewhere.  A ray whose row is NaN (its member had no
    render term, or the ray was already absent) keeps 1: nothing is known against it."""
    sdf = np.asarray(report["pt_sdf"])
    alive = np.asarray(report["pt_alive"], bool)
    res = np.asarray(report["ray_residual"])
    with np.errstate(invalid="ignore"):
        pt_w = np.where((np.abs(sdf) > float(pt_sdf_max)) | ~alive, 0.0, 1.0).astype(np.float32)
        ray_w = np.where(np.abs(res) > float(ray_res_max), 0.0, 1.0).astype(np.float32)
    return pt_w, ray_w
