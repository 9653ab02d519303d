"""ORACLE -- CPU restatement (numpy, float32) of DSP-SLAM's DeepSDF shape/pose Gauss-Newton path.

THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, __graft_entry__.smoke() and the
`cpu_baseline` leg of bench.py may import it; the shipped path (dsp_slam_amd/) never does and
fails loudly when the HIP library is missing.

Every function restates one reference function and cites the file:line it follows (paths are
relative to the reference tree).  Parity status: PINNED -- the reference has no tests or golden
vectors of its own, so this oracle is pinned against outputs of the
UNMODIFIED reference Python run on CPU in the build container (tools/make_golden.py ->
tests/golden/*.npz; checked by tests/test_oracle_golden.py).

Arithmetic is float32 throughout, like the reference (torch default dtype).  Dense products go
through `_mm`, which uses a BLAS sgemm (torch CPU when importable -- ~6x faster than numpy's
bundled OpenBLAS on this image -- else numpy); that is a choice of BLAS, not of algorithm.
"""
import math
import os

import numpy as np

F32 = np.float32

_BLAS = os.environ.get("DSP_ORACLE_BLAS", "auto")
_torch = None
if _BLAS in ("auto", "torch"):
    try:
        import torch as _torch  # noqa: N812  (sgemm provider only)
    except Exception:  # pragma: no cover
        _torch = None


def _mm(a, b):
    """(n,k) @ (k,m) float32 sgemm."""
    a = np.ascontiguousarray(a, dtype=F32)
    b = np.ascontiguousarray(b, dtype=F32)
    if _torch is not None and a.shape[0] >= 64:
        return _torch.mm(_torch.from_numpy(a), _torch.from_numpy(b)).numpy()
    return a @ b


# ----------------------------------------------------------------------------------------------
# Decoder  (deep_sdf/deep_sdf_decoder.py:9-110, deep_sdf/workspace.py:202-223)
# ----------------------------------------------------------------------------------------------
class FoldedDecoder(object):
    """Weight-norm-folded DeepSDF MLP.  layers[k] = (W (out,in) f32, b (out,) f32)."""

    def __init__(self, layers, latent_in, code_len):
        self.layers = layers
        self.latent_in = tuple(latent_in)
        self.code_len = int(code_len)
        self.in_dim = self.code_len + 3


def fold_decoder(state_dict, specs):
    """state_dict keyed like Decoder.state_dict() (optional `module.` prefix), numpy or torch values.

    Folds nn.utils.weight_norm: W = g * v / ||v||_2 per output row (deep_sdf_decoder.py:49-54).
    Layer shapes follow deep_sdf_decoder.py:27-47 (layer k+1 in latent_in => out_dim -= dims[0]).
    """
    ns = specs["NetworkSpecs"]
    if ns.get("xyz_in_all") or ns.get("use_tanh") or ns.get("latent_dropout"):
        raise NotImplementedError("only the DSP-SLAM decoder configuration is restated")
    if not ns.get("weight_norm") and ns.get("norm_layers"):
        raise NotImplementedError("LayerNorm variant (weight_norm=False) not restated")
    sd = {}
    for k, v in state_dict.items():
        a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        sd[k[7:] if k.startswith("module.") else k] = a.astype(F32)
    n_lin = len(ns["dims"]) + 1
    layers = []
    for k in range(n_lin):
        name = "lin%d" % k
        if name + ".weight_v" in sd:
            v = sd[name + ".weight_v"]
            g = sd[name + ".weight_g"].reshape(-1, 1)
            nrm = np.sqrt((v.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(F32)
            w = (v * (g / nrm)).astype(F32)  # torch._weight_norm: v * (g / norm)
        else:
            w = sd[name + ".weight"]
        layers.append((np.ascontiguousarray(w, dtype=F32), sd[name + ".bias"].astype(F32)))
    return FoldedDecoder(layers, ns["latent_in"], specs["CodeLength"])


def decoder_forward(dec, x, keep=False):
    """Decoder.forward (deep_sdf_decoder.py:75-110): x (N, code_len+3) -> y (N,).

    With keep=True also returns the pre-activations needed by the backward restatement.
    """
    x = np.ascontiguousarray(x, dtype=F32)
    h = x
    pre = []
    n_lin = len(dec.layers)
    for k, (w, b) in enumerate(dec.layers):
        if k in dec.latent_in:
            h = np.concatenate([h, x], axis=-1)              # :89-90
        a = _mm(h, w.T) + b                                   # :93
        if keep:
            pre.append(a)
        h = np.maximum(a, F32(0)) if k < n_lin - 1 else a    # :97-104 (relu; LayerNorm/dropout inert)
    y = np.tanh(h[:, 0]).astype(F32)                          # :107-108
    return (y, pre) if keep else y


def decoder_forward_backward(dec, x):
    """y and dy/dx -- what get_batch_sdf_jacobian's autograd call yields
    (reconstruct/loss_utils.py:82-103)."""
    x = np.ascontiguousarray(x, dtype=F32)
    y, pre = decoder_forward(dec, x, keep=True)
    n_lin = len(dec.layers)
    g = ((F32(1) - y * y)[:, None] * dec.layers[-1][0]).astype(F32)   # d tanh * W8 -> (N, 512)
    g_skip = np.zeros_like(x)
    for k in range(n_lin - 2, -1, -1):
        w = dec.layers[k][0]
        g = g * (pre[k] > 0)                                   # relu'(0) = 0
        g = _mm(g, w)                                          # (N, in_k)
        if k in dec.latent_in:
            g_skip = g_skip + g[:, -dec.in_dim:]
            g = g[:, :-dec.in_dim]
    return y, (g + g_skip).astype(F32)


def decode_sdf(dec, code, pts, max_batch=64 ** 3):
    """reconstruct/loss_utils.py:51-79 -- no-grad forward in chunks; code (C,), pts (N,3) -> (N,)."""
    pts = np.ascontiguousarray(pts, dtype=F32)
    out = []
    for head in range(0, pts.shape[0], max_batch):
        sub = pts[head:head + max_batch]
        x = np.concatenate([np.broadcast_to(code.astype(F32), (sub.shape[0], code.shape[0])), sub], -1)
        out.append(decoder_forward(dec, x))
    return np.concatenate(out, 0) if out else np.zeros((0,), F32)


def get_batch_sdf_jacobian(dec, code, pts):
    """reconstruct/loss_utils.py:82-103 -> y (N,), dy/d[code,xyz] (N, C+3)."""
    pts = np.ascontiguousarray(pts, dtype=F32)
    if pts.shape[0] == 0:
        return np.zeros((0,), F32), np.zeros((0, dec.in_dim), F32)
    x = np.concatenate([np.broadcast_to(code.astype(F32), (pts.shape[0], code.shape[0])), pts], -1)
    return decoder_forward_backward(dec, x)


# ----------------------------------------------------------------------------------------------
# Lie-group helpers  (reconstruct/loss_utils.py:107-233)
# ----------------------------------------------------------------------------------------------
def points_to_pose_jacobian_se3(p):
    """loss_utils.py:107-126: (N,3) -> (N,3,6) = [I | -[p]x]."""
    n = p.shape[0]
    j = np.zeros((n, 3, 6), F32)
    j[:, 0, 0] = j[:, 1, 1] = j[:, 2, 2] = 1
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    j[:, 0, 4] = z
    j[:, 0, 5] = -y
    j[:, 1, 3] = -z
    j[:, 1, 5] = x
    j[:, 2, 3] = y
    j[:, 2, 4] = -x
    return j


def points_to_pose_jacobian_sim3(p):
    """loss_utils.py:166-185: (N,3) -> (N,3,7) = [I | -[p]x | p]."""
    return np.concatenate([points_to_pose_jacobian_se3(p), p[:, :, None].astype(F32)], axis=-1)


# torch's float32 exp / sin / cos on the CPU (Sleef u10) return the correctly rounded value for 99 % / 95 % / 95 % of arguments; numpy's float32
# exp does so for only 60 %.  The difference matters: exp_sim3 forms c = (e^s - 1) / s, which amplifies the last bit of e^s by 1 / s (s = 1e-6:
# one ulp of e^s is 12 % of c).  Rounding the float64 value is the closest restatement of the reference's arithmetic that does not copy Sleef.
def _exp32(x):
    return F32(np.exp(np.float64(x)))


def _sin32(x):
    return F32(np.sin(np.float64(x)))


def _cos32(x):
    return F32(np.cos(np.float64(x)))


def _hat(w):
    return np.array([[0., -w[2], w[1]], [w[2], 0., -w[0]], [-w[1], w[0], 0.]], F32)


def exp_se3(x):
    """loss_utils.py:129-163 (float32, as torch on CPU)."""
    x = np.asarray(x, F32)
    v, w = x[:3], x[3:6]
    w_hat = _hat(w)
    w_hat2 = (w_hat @ w_hat).astype(F32)
    theta = F32(np.sqrt(np.sum(w * w, dtype=F32)))
    eye = np.eye(3, dtype=F32)
    if theta <= 1e-8:
        e_w, j = eye, eye
    else:
        s, c = _sin32(theta), _cos32(theta)
        t2, t3 = F32(theta ** 2), F32(theta ** 3)
        e_w = eye + w_hat * s / theta + w_hat2 * (F32(1.) - c) / t2
        k1 = (F32(1) - c) / t2
        k2 = (theta - s) / t3
        j = eye + k1 * w_hat + k2 * w_hat2
    rst = np.eye(4, dtype=F32)
    rst[:3, :3] = e_w
    rst[:3, 3] = (j.astype(F32) @ v).astype(F32)
    return rst


def exp_sim3(x):
    """loss_utils.py:188-233, quirks included: c = 0 when s <= 1e-8 in the theta > 1e-8 branch (:223)."""
    x = np.asarray(x, F32)
    v, w, s = x[:3], x[3:6], F32(x[6])
    w_hat = _hat(w)
    w_hat2 = (w_hat @ w_hat).astype(F32)
    theta = F32(np.sqrt(np.sum(w * w, dtype=F32)))
    t2 = F32(theta ** 2)
    sn, cs = _sin32(theta), _cos32(theta)
    e_s = _exp32(s)
    s2 = F32(s ** 2)
    eye = np.eye(3, dtype=F32)
    eps = 1e-8
    if theta <= 1e-8:
        e_w = eye
        if s == 0:
            j = eye
        else:
            j = ((e_s - F32(1.)) / s) * eye
    else:
        e_w = eye + w_hat * sn / theta + w_hat2 * (F32(1.) - cs) / t2
        a = e_s * sn
        b = e_s * cs
        c = F32(0.) if s <= eps else (e_s - F32(1.)) / s
        k0 = c * eye
        k1 = (a * s + (F32(1) - b) * theta) / (s2 + t2)
        k2 = c - ((b - F32(1)) * s + a * theta) / (s2 + t2)
        j = k0 + k1 * w_hat / theta + k2 * w_hat2 / t2
    rst = np.eye(4, dtype=F32)
    rst[:3, :3] = (e_s * e_w).astype(F32)
    rst[:3, 3] = (j.astype(F32) @ v).astype(F32)
    return rst


def _inv(a):
    """torch.inverse on CPU float32 == LAPACK sgetrf-based inverse; numpy float32 inv is the same class."""
    return np.linalg.inv(np.asarray(a, F32)).astype(F32)


def _det3_cuberoot(r):
    """torch.det(R) ** (1/3) in float32 (optimizer.py:122, loss.py:163)."""
    d = F32(np.linalg.det(np.asarray(r, F32)))
    return F32(np.power(d, F32(1.0 / 3.0)))


def linspace_f32(start, end, steps):
    """torch.linspace on CPU float32: step = (end-start)/(steps-1); first half start + i*step,
    second half end - (steps-1-i)*step (ATen RangeFactories linspace kernel)."""
    start, end = F32(start), F32(end)
    step = F32((end - start) / F32(steps - 1))
    i = np.arange(steps)
    lo = (start + step * i.astype(F32)).astype(F32)
    hi = (end - step * (steps - 1 - i).astype(F32)).astype(F32)
    return np.where(i < steps // 2, lo, hi).astype(F32)


# ----------------------------------------------------------------------------------------------
# Robust kernel  (reconstruct/loss_utils.py:236-265)
# ----------------------------------------------------------------------------------------------
def huber_norm_weights(x, b):
    """loss_utils.py:236-248: x = |r| (N,), w = sqrt(rho(x)) / x, w(0) = 0."""
    x = np.asarray(x, F32).copy()
    b = F32(b)
    rho = np.where(x <= b, x * x, F32(2) * b * x - b * b).astype(F32)
    x[x == 0] = 1.
    return (np.sqrt(rho) / x).astype(F32)


def get_robust_res(res, b):
    """loss_utils.py:251-265 -> (w*res, mean((w*res)^2), w).  Empty input => loss NaN, like torch.mean."""
    res = np.asarray(res, F32).reshape(-1)
    w = huber_norm_weights(np.abs(res), b)
    rr = (w * res).astype(F32)
    loss = F32(np.mean(rr * rr, dtype=F32)) if rr.size else F32(np.nan)
    return rr, loss, w


# ----------------------------------------------------------------------------------------------
# Residual terms  (reconstruct/loss.py)
# ----------------------------------------------------------------------------------------------
def transform_points(t_obj_cam, p):
    """(p[..., None, :] * R).sum(-1) + t  (loss.py:31-32, 62-63), float32, products summed in column order."""
    r = np.asarray(t_obj_cam, F32)[:3, :3]
    t = np.asarray(t_obj_cam, F32)[:3, 3]
    p = np.asarray(p, F32)
    out = np.empty(p.shape, F32)
    for i in range(3):
        acc = (p[..., 0] * r[i, 0]).astype(F32)
        acc = (acc + (p[..., 1] * r[i, 1]).astype(F32)).astype(F32)
        acc = (acc + (p[..., 2] * r[i, 2]).astype(F32)).astype(F32)
        out[..., i] = acc + t[i]
    return out


def compute_sdf_loss(dec, pts_surface_cam, t_obj_cam, code):
    """loss.py:22-43 -> J_pose (N,7), J_code (N,C), residual (N,)."""
    p_o = transform_points(t_obj_cam, pts_surface_cam)
    res, de_di = get_batch_sdf_jacobian(dec, code, p_o)
    de_dxo = de_di[:, -3:]
    dxo = points_to_pose_jacobian_sim3(p_o)
    jac_toc = np.einsum("ni,nij->nj", de_dxo, dxo).astype(F32)
    return jac_toc, de_di[:, :-3], res


def sdf_to_occupancy(sdf, th):
    """loss_utils.py:40-48."""
    th = F32(th)
    return (F32(0.5) - np.clip(sdf, -th, th) / (F32(2) * th)).astype(F32)


def compute_render_loss(dec, ray_directions, depth_obs, t_obj_cam, sampled_ray_depth, code, th=0.01,
                        stats=None, sdf_jitter=0.0):
    """loss.py:46-152 -> (J_pose (K,7), J_code (K,C), residual (K,)) or None (<10 in-sphere samples).

    stats (optional dict) receives the ragged set sizes V, m, K and the index sets.
    """
    rays = np.asarray(ray_directions, F32)
    d = np.asarray(sampled_ray_depth, F32)
    th = F32(th)
    n_rays, n_d = rays.shape[0], d.shape[0]
    pts_cam = (rays[:, None, :] * d[None, :, None]).astype(F32)          # :60
    pts_obj = transform_points(t_obj_cam, pts_cam)                          # :62-63
    nrm = np.sqrt(np.sum(pts_obj * pts_obj, axis=-1, dtype=F32)).astype(F32)
    vx, vy = np.where(nrm < F32(1.0))                                       # :68 (row-major order)
    query = pts_obj[vx, vy, :]
    if stats is not None:
        stats["V"] = int(query.shape[0])
    if query.shape[0] < 10:                                                 # :73-74
        return None
    sdf = decode_sdf(dec, code, query)                                      # :77-78
    if sdf_jitter:   # tests only: +-jitter on the decoded values, to measure how round-off in the decoder propagates
        sdf = (sdf + F32(sdf_jitter) * np.where(np.arange(sdf.shape[0]) % 2 == 0, F32(1), F32(-1))).astype(F32)
    occ = np.zeros((n_rays, n_d), F32)
    occ[vx, vy] = sdf_to_occupancy(sdf, th)                                 # :84-86
    wg = (sdf > -th) & (sdf < th)                                           # :88
    gx, gy = vx[wg], vy[wg]
    occ_g = occ[gx, :]                                                      # (m, D)  :93
    m = occ_g.shape[0]
    d_min, d_max = d[0], d[-1]
    acc = np.cumprod(F32(1) - occ_g, axis=-1, dtype=F32)                    # :99
    acc_aug = np.concatenate([np.ones((m, 1), F32), acc], -1)
    o = np.concatenate([occ_g, np.ones((m, 1), F32)], -1)
    dd = np.concatenate([d, np.array([F32(1.1) * d_max], F32)], -1)
    term = (o * acc_aug).astype(F32)
    d_u = np.sum(dd * term, axis=-1, dtype=F32)                             # :112-114
    o_k = occ[gx, gy]
    l_idx = np.arange(n_d)[None, :]
    acc_z = np.where(l_idx < gy[:, None], F32(0), acc)                      # :121
    de_do = (np.sum(acc_z, axis=-1, dtype=F32) / (F32(1.) - o_k)).astype(F32)
    nz = de_do > F32(1e-2)                                                  # :125
    if stats is not None:      # forensics: everything a threshold decision was made on (tests name flipped samples by these)
        stats.update(norm=nrm, band=(gx.copy(), gy.copy()), de_do_band=de_do.copy())
    de_do = de_do[nz]
    d_u = d_u[nz]
    delta_d = F32((d_max - d_min) / F32(n_d - 1))
    do_ds = F32(-1.) / (F32(2) * th)
    de_ds = (de_do * delta_d * do_ds).astype(F32)                           # :130
    gx, gy = gx[nz], gy[nz]
    res = (np.asarray(depth_obs, F32)[gx] - d_u).astype(F32)                # :135-136
    res = np.clip(res, F32(-0.30), F32(0.30))                               # :139-140
    pts_g = pts_obj[gx, gy]
    _, ds_di = get_batch_sdf_jacobian(dec, code, pts_g)                     # :144
    de_di = (de_ds[:, None] * ds_di).astype(F32)
    dxo = points_to_pose_jacobian_sim3(pts_g)
    jac_toc = np.einsum("ni,nij->nj", de_di[:, -3:], dxo).astype(F32)
    if stats is not None:
        stats.update(m=int(m), K=int(gx.shape[0]), valid=(vx, vy), kept=(gx, gy), sdf=sdf, de_ds=de_ds)
    return jac_toc, de_di[:, :-3], res


def compute_rotation_loss_sim3(t_obj_cam):
    """loss.py:155-178 (CPU float32) -> (J (7,), residual)."""
    t_cam_obj = _inv(t_obj_cam)
    r_co = t_cam_obj[:3, :3].copy()
    scale = _det3_cuberoot(r_co)
    r_co = (r_co / scale).astype(F32)
    r_oc = _inv(r_co)
    ey = np.array([0., 1., 0.], F32)
    ng = np.array([0., -1., 0.], F32)
    ry = (r_co @ ey).astype(F32)
    res = F32(1.) - F32(np.dot(ry, ng))
    if res < 1e-7:
        return np.zeros(7, F32), F32(0.)
    j = np.zeros(7, F32)
    j[3:6] = np.cross((r_oc @ ng).astype(F32), ey).astype(F32)
    return j, res


# ----------------------------------------------------------------------------------------------
# Optimiser  (reconstruct/optimizer.py)
# ----------------------------------------------------------------------------------------------
class GNParams(object):
    """Hyper-parameters read by Optimizer.__init__ (optimizer.py:27-43)."""

    def __init__(self, k1=1.0, k2=100.0, k3=0.25, k4=1e7, b1=0.2, b2=0.025, lr=1.0, s_damp=1.0,
                 num_iterations=10, code_len=64, num_depth_samples=50, cut_off=0.01,
                 num_iterations_pose_only=5):
        self.k1, self.k2, self.k3, self.k4 = k1, k2, k3, k4
        self.b1, self.b2, self.lr, self.s_damp = b1, b2, lr, s_damp
        self.num_iterations = num_iterations
        self.code_len = code_len
        self.num_depth_samples = num_depth_samples
        self.cut_off = cut_off
        self.num_iterations_pose_only = num_iterations_pose_only

    @classmethod
    def from_configs(cls, cfg):
        o = cfg["optimizer"]
        j = o["joint_optim"]
        p = o.get("pose_only_optim", {"num_iterations": 5})
        return cls(j["k1"], j["k2"], j["k3"], j["k4"], j["b1"], j["b2"], j["learning_rate"],
                   j["scale_damping"], j["num_iterations"], o["code_len"], o["num_depth_samples"],
                   o["cut_off_threshold"], p["num_iterations"])


def set_checksum(ray_idx, depth_idx):
    """Order-independent checksum of a sample set, same definition as the device's (include/dsp_gn.h, dsp_batch_trace)."""
    ids = (np.asarray(ray_idx, np.uint64) << np.uint64(6)) | np.asarray(depth_idx, np.uint64)
    ids = ids & np.uint64(0xFFFFFFFF)
    h = ((ids * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) ^ (ids >> np.uint64(7))
    return int(h.sum() & np.uint64(0xFFFFFFFF)) if ids.size else 0


def _gram(j, r):
    """sum_n J_n^T J_n and sum_n J_n^T r_n for row Jacobians (optimizer.py:162-167)."""
    j = np.ascontiguousarray(j, F32)
    return (j.T @ j).astype(F32), (j.T @ np.asarray(r, F32)).astype(F32)


def reconstruct_object(dec, prm, t_cam_obj, pts, rays, depth, code=None, trace=None, t_obj_cam0=None, sdf_jitter=0.0,
                       scale_jitter=0.0, sampled_override=None):
    """Optimizer.reconstruct_object (optimizer.py:88-203).

    Returns dict(t_cam_obj (4,4) f32 | None, code (C,) f32 | None, is_good bool, loss float).
    trace (optional list) receives one dict per GN iteration.
    """
    c_len = prm.code_len
    z = np.zeros(c_len, F32) if code is None else np.asarray(code, F32)[:c_len].copy()
    # t_obj_cam0 (tests only): start from a given camera->object matrix instead of inverting t_cam_obj
    t_obj_cam = _inv(np.asarray(t_cam_obj, F32)) if t_obj_cam0 is None else np.asarray(t_obj_cam0, F32).copy()
    rays = np.asarray(rays, F32)
    depth = np.asarray(depth, F32)
    n_fg = depth.shape[0]
    n_bg = rays.shape[0] - n_fg
    depth_obs = np.concatenate([depth, np.zeros(n_bg, F32)]).astype(F32)
    pts = np.asarray(pts, F32)
    loss = 0.
    fail = lambda: dict(t_cam_obj=None, code=None, is_good=False, loss=loss)  # noqa: E731
    for e in range(prm.num_iterations):
        t_co = _inv(t_obj_cam)                                               # :120
        scale = _det3_cuberoot(t_co[:3, :3])                                 # :122
        if scale_jitter:   # tests only: the derived scale moved by a relative round-off (fp32 det/pow vs other exact paths)
            scale = F32(scale * F32(1.0 + scale_jitter))
        d_min = F32(t_co[2, 3] - F32(1.0) * scale)
        d_max = F32(t_co[2, 3] + F32(1.0) * scale)
        sampled = linspace_f32(d_min, d_max, prm.num_depth_samples)          # :125
        if sampled_override is not None:   # tests only: linearise on exactly these depth samples (one row per iteration, or one row for a single-iteration run)
            so = np.asarray(sampled_override, F32)
            sampled = (so[e] if so.ndim == 2 else so)[:prm.num_depth_samples].copy()
            d_max = sampled[-1]
        derived_depths = sampled.copy()
        depth_obs[n_fg:] = F32(1.1) * d_max                                  # :126
        j7_s, jc_s, r_s = compute_sdf_loss(dec, pts, t_obj_cam, z)           # :129
        rr_s, sdf_loss, _ = get_robust_res(r_s, prm.b2)                      # :134
        if math.isnan(sdf_loss):
            return fail()
        st = {}
        rend = compute_render_loss(dec, rays, depth_obs, t_obj_cam, sampled, z, th=prm.cut_off, stats=st, sdf_jitter=sdf_jitter)
        if rend is None:                                                     # :142-143
            return fail()
        j7_r, jc_r, r_r = rend
        rr_r, render_loss, _ = get_robust_res(r_r, prm.b1)                   # :148
        if math.isnan(render_loss):
            return fail()
        j_rot, res_rot = compute_rotation_loss_sim3(t_obj_cam)               # :153
        loss = float(F32(prm.k1) * render_loss + F32(prm.k2) * sdf_loss)     # :155
        pd = 7
        j_s = np.concatenate([j7_s, jc_s], -1)
        hs, bs = _gram(j_s, rr_s)
        h_sdf = (F32(prm.k2) * hs / F32(j_s.shape[0])).astype(F32)           # :162
        b_sdf = (-F32(prm.k2) * bs / F32(j_s.shape[0])).astype(F32)
        j_r = np.concatenate([j7_r, jc_r], -1)
        hr, br = _gram(j_r, rr_r)
        h_r = (F32(prm.k1) * hr / F32(j_r.shape[0])).astype(F32)             # :166
        b_r = (-F32(prm.k1) * br / F32(j_r.shape[0])).astype(F32)
        h = (h_r + h_sdf).astype(F32)
        h[pd:, pd:] += F32(prm.k3) * np.eye(c_len, dtype=F32)                # :170
        b = (b_r + b_sdf).astype(F32)
        b[pd:] -= F32(prm.k3) * z                                            # :172
        h_rot = np.outer(j_rot, j_rot).astype(F32)                           # :176
        b_rot = -(j_rot * res_rot).astype(F32)                               # :177
        h[:pd, :pd] += F32(prm.k4) * h_rot
        b[:pd] -= F32(prm.k4) * b_rot                                        # :179 (sign as written)
        h[:pd, :pd] += np.eye(pd, dtype=F32)                                 # :183
        h[pd - 1, pd - 1] += F32(prm.s_damp)                                 # :184
        dx = (_inv(h) @ b).astype(F32)                                       # :186
        delta_t = exp_sim3(F32(prm.lr) * dx[:pd])                            # :190
        if trace is not None:
            trace.append(dict(V=st["V"], m=st["m"], K=st["K"], vsum=set_checksum(*st["valid"]), ksum=set_checksum(*st["kept"]), sets=st,
                              H=h.copy(), b=b.copy(), dx=dx.copy(), depths=derived_depths,
                              t_obj_cam=t_obj_cam.copy(), code=z.copy(), loss=loss,
                              sdf_loss=float(sdf_loss), render_loss=float(render_loss)))
        t_obj_cam = (delta_t @ t_obj_cam).astype(F32)                        # :191
        z = (z + F32(prm.lr) * dx[pd:pd + c_len]).astype(F32)                # :192
    return dict(t_cam_obj=_inv(t_obj_cam), code=z, is_good=True, loss=loss)


# ----------------------------------------------------------------------------------------------
# float64 linearisation (the yardstick of tests/gn_metric.py; not a restatement of the reference's rounding)
# ----------------------------------------------------------------------------------------------
F64 = np.float64


def _mm64(a, b):
    """(n,k) @ (k,m) float64 dgemm."""
    a = np.ascontiguousarray(a, dtype=F64)
    b = np.ascontiguousarray(b, dtype=F64)
    if _torch is not None and a.shape[0] >= 64:
        return _torch.mm(_torch.from_numpy(a), _torch.from_numpy(b)).numpy()
    return a @ b


# A hidden pre-activation may land on the other side of its ReLU in an fp32 implementation when it lies within that implementation's
# round-off of zero.  Its round-off has two parts: the fp32 dot product itself (a few ulp of sum_i |w_i h_i| + |b|) and the rounding of
# the transformed point (a few ulp of each coordinate) carried to the unit by d a / d xyz.  RELU_ULPS of both is the band.
RELU_ULPS = 2.0
EPS32 = 2.0 ** -24


def _decoder_fb64(dec, x, grad=True, dp=None):
    """decoder_forward_backward in float64 on the float32 weights (cast exactly) -> y (N,), dy/dx (N, in_dim) or None, and dy/dx with
    the ReLU mask flipped at every hidden unit whose pre-activation lies within its fp32 round-off band of zero (the gradient on the
    other side of the kink, which an fp32 implementation may take; equal to dy/dx in rows without such a unit) or None.
    dp (N, 3): the rounding scale of each point coordinate (see RELU_ULPS)."""
    x = np.ascontiguousarray(x, dtype=F64)
    n, n_lin = x.shape[0], len(dec.layers)
    h, pre, near = x, [], []
    t_x = np.zeros((3, n, x.shape[1]))                      # d x / d xyz
    for d in range(3):
        t_x[d, :, x.shape[1] - 3 + d] = 1.0
    t_h = t_x
    for k, (w, b) in enumerate(dec.layers):
        w64 = w.astype(F64)
        if k in dec.latent_in:
            h = np.concatenate([h, x], axis=-1)
            t_h = np.concatenate([t_h, t_x], axis=-1)
        a = _mm64(h, w64.T) + b.astype(F64)
        pre.append(a)
        if grad and k < n_lin - 1:
            band = EPS32 * (_mm64(np.abs(h), np.abs(w64).T) + np.abs(b.astype(F64)))
            t_a = np.stack([_mm64(t_h[d], w64.T) for d in range(3)])
            if dp is not None:
                band = band + sum(np.abs(t_a[d]) * dp[:, d:d + 1] for d in range(3))
            near.append(np.abs(a) <= RELU_ULPS * band)
            t_h = t_a * (a > 0)
        h = np.maximum(a, 0.0) if k < n_lin - 1 else a
    y = np.tanh(h[:, 0])
    if not grad:
        return y, None, None

    def backward(flip):
        g = (1.0 - y * y)[:, None] * dec.layers[-1][0].astype(F64)
        g_skip = np.zeros_like(x)
        for k in range(n_lin - 2, -1, -1):
            m = pre[k] > 0
            if flip:
                m = m ^ near[k]
            g = _mm64(g * m, dec.layers[k][0].astype(F64))
            if k in dec.latent_in:
                g_skip = g_skip + g[:, -dec.in_dim:]
                g = g[:, :-dec.in_dim]
        return g + g_skip

    g = backward(False)
    return y, g, (backward(True) if any(m.any() for m in near) else g)


def _decode64(dec, code, p, grad=True, chunk=4096, dp=None):
    """(sdf (N,), d sdf / d[code, xyz] (N, C+3) or None, the same with near-zero ReLUs flipped or None) at float64 points p (N, 3)."""
    n = p.shape[0]
    ys, gs, gf = [np.zeros(0, F64)], [np.zeros((0, dec.in_dim), F64)], [np.zeros((0, dec.in_dim), F64)]
    for h in range(0, n, chunk):
        sub = p[h:h + chunk]
        x = np.concatenate([np.broadcast_to(np.asarray(code, F64), (sub.shape[0], dec.code_len)), sub], -1)
        y, g, g2 = _decoder_fb64(dec, x, grad, None if dp is None else dp[h:h + chunk])
        ys.append(y)
        if grad:
            gs.append(g)
            gf.append(g2)
    if not grad:
        return np.concatenate(ys), None, None
    return np.concatenate(ys), np.concatenate(gs), np.concatenate(gf)


def _flip_allowance(j, j_alt, rr, w):
    """Entrywise |change| of w sum_n J_n^T J_n and of w sum_n J_n r_n when the rows j take their other-side-of-the-kink values j_alt,
    summed over the rows that differ -> (A_H, a_b, number of rows)."""
    rows = np.where(np.any(j_alt != j, axis=1))[0]
    n = j.shape[1]
    a_h, a_b = np.zeros((n, n)), np.zeros(n)
    for r in rows:
        a_h += w * np.abs(np.outer(j_alt[r], j_alt[r]) - np.outer(j[r], j[r]))
        a_b += w * np.abs((j_alt[r] - j[r]) * rr[r])
    return a_h, a_b, int(rows.shape[0])


def _robust_rows64(res, b):
    """get_robust_res's w * res in float64."""
    x = np.abs(res)
    rho = np.where(x <= b, x * x, 2.0 * b * x - b * b)
    w = np.sqrt(rho) / np.where(x == 0, 1.0, x)
    return w * res


def _sim3_rows64(p):
    """points_to_pose_jacobian_sim3 in float64: (N,3) -> (N,3,7)."""
    n = p.shape[0]
    j = np.zeros((n, 3, 7), F64)
    j[:, 0, 0] = j[:, 1, 1] = j[:, 2, 2] = 1
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    j[:, 0, 4], j[:, 0, 5] = z, -y
    j[:, 1, 3], j[:, 1, 5] = -z, x
    j[:, 2, 3], j[:, 2, 4] = y, -x
    j[:, :, 6] = p
    return j


def _view_rows64(dec, prm, pts, rays, depth, t_view, code, depths, sets):
    """The float64 rows one view contributes to a Gauss-Newton system at its camera->object matrix t_view (loss.py:22-152): a dict of
    j_s / j_r (surface and render jacobian rows, (n, 7 + code_len)), j_s2 / j_r2 (their twins on the other side of every ReLU kink within
    round-off, _decoder_fb64), r_s / r_r (the robust residuals w * r of get_robust_res) and V, K, N.  sets as in linearise_fp64; a view
    with an empty `kept` set, without rays or without points gives zero rows of that kind."""
    c_len = prm.code_len
    z = np.asarray(code, F64)[:c_len]
    t = np.asarray(t_view, F32).astype(F64)
    r_m, t_v = t[:3, :3], t[:3, 3]
    rays = np.asarray(rays, F32).astype(F64).reshape(-1, 3)
    d = np.asarray(depths, F32).astype(F64)[:prm.num_depth_samples]
    n_d = d.shape[0]
    n_fg = np.asarray(depth).reshape(-1).shape[0]
    d_min, d_max = d[0], d[-1]
    c11 = float(F32(1.1))                                     # the reference's constants are float32 scalars
    depth_obs = np.concatenate([np.asarray(depth, F32).astype(F64).reshape(-1), np.full(rays.shape[0] - n_fg, c11 * d_max)])
    th = float(F32(prm.cut_off))
    # surface term (loss.py:22-43)
    p_in = np.asarray(pts, F32).astype(F64).reshape(-1, 3)
    p_s = p_in @ r_m.T + t_v
    r_s, g_s, g_s2 = _decode64(dec, z, p_s, dp=EPS32 * (np.abs(p_in) @ np.abs(r_m).T + np.abs(t_v)))
    sim_s = _sim3_rows64(p_s)
    j_s = np.concatenate([np.einsum("ni,nij->nj", g_s[:, -3:], sim_s), g_s[:, :-3]], -1)
    j_s2 = np.concatenate([np.einsum("ni,nij->nj", g_s2[:, -3:], sim_s), g_s2[:, :-3]], -1)
    rr_s = _robust_rows64(r_s, float(F32(prm.b2)))
    # render term (loss.py:46-152) on the given sets
    vx, vy = (np.asarray(a, np.int64).reshape(-1) for a in sets["valid"])
    gx, gy = (np.asarray(a, np.int64).reshape(-1) for a in sets["kept"])
    p_v = (rays[vx] * d[vy, None]) @ r_m.T + t_v
    sdf_v = _decode64(dec, z, p_v, grad=False)[0]
    occ = np.zeros((rays.shape[0], n_d), F64)
    occ[vx, vy] = 0.5 - np.clip(sdf_v, -th, th) / (2.0 * th)
    occ_g = occ[gx]                                           # (K, D): the kept rows' rays
    acc = np.cumprod(1.0 - occ_g, axis=-1)
    acc_aug = np.concatenate([np.ones((gx.shape[0], 1)), acc], -1)
    o = np.concatenate([occ_g, np.ones((gx.shape[0], 1))], -1)
    dd = np.concatenate([d, [c11 * d_max]])
    d_u = np.sum(dd * o * acc_aug, axis=-1)
    o_k = occ[gx, gy]
    acc_z = np.where(np.arange(n_d)[None, :] < gy[:, None], 0.0, acc)
    de_do = np.sum(acc_z, axis=-1) / (1.0 - o_k)
    de_ds = de_do * ((d_max - d_min) / (n_d - 1)) * (-1.0 / (2.0 * th))
    r_r = np.clip(depth_obs[gx] - d_u, -float(F32(0.30)), float(F32(0.30)))
    p_k = (rays[gx] * d[gy, None]) @ r_m.T + t_v
    p_cam = rays[gx] * d[gy, None]
    _, ds_di, ds_di2 = _decode64(dec, z, p_k, dp=EPS32 * (2 * np.abs(p_cam) @ np.abs(r_m).T + np.abs(t_v)))
    sim_k = _sim3_rows64(p_k)
    de_di, de_di2 = de_ds[:, None] * ds_di, de_ds[:, None] * ds_di2
    j_r = np.concatenate([np.einsum("ni,nij->nj", de_di[:, -3:], sim_k), de_di[:, :-3]], -1)
    j_r2 = np.concatenate([np.einsum("ni,nij->nj", de_di2[:, -3:], sim_k), de_di2[:, :-3]], -1)
    rr_r = _robust_rows64(r_r, float(F32(prm.b1)))
    return dict(j_s=j_s, j_s2=j_s2, r_s=rr_s, j_r=j_r, j_r2=j_r2, r_r=rr_r, V=int(vx.shape[0]), K=int(j_r.shape[0]), N=int(j_s.shape[0]))


def _assemble64(prm, rows, t_obj_cam, code):
    """The Gauss-Newton system of optimizer.py:153-186 in float64 from the rows of any number of views (_view_rows64), pooled as one row
    set: data Grams and gradients over the pooled N and K, the losses and the kink allowances from the pooled rows, and the code prior,
    rotation prior and damping once, at the object's own t_obj_cam.  A row kind nobody contributes to leaves its terms at zero."""
    c_len = prm.code_len
    z = np.asarray(code, F64)[:c_len]
    t = np.asarray(t_obj_cam, F32).astype(F64)
    pd = 7
    n_unk = pd + c_len
    one = len(rows) == 1
    j_s, j_s2, rr_s, j_r, j_r2, rr_r = ((rows[0][k] if one else np.concatenate([r[k] for r in rows])) for k in ("j_s", "j_s2", "r_s", "j_r", "j_r2", "r_r"))
    # rotation prior (loss.py:155-178)
    t_co = np.linalg.inv(t)
    r_co = t_co[:3, :3] / np.cbrt(np.linalg.det(t_co[:3, :3]))
    res_rot = 1.0 + r_co[1, 1]
    j_rot = np.zeros(pd)
    if res_rot >= 1e-7:
        j_rot[3:6] = np.cross(np.linalg.inv(r_co) @ np.array([0., -1., 0.]), np.array([0., 1., 0.]))
    else:
        res_rot = 0.0
    k1, k2, k3, k4 = (float(F32(v)) for v in (prm.k1, prm.k2, prm.k3, prm.k4))
    n_s, n_k = j_s.shape[0], j_r.shape[0]
    if n_s:
        sdf_loss = float(np.mean(rr_s * rr_s))
        ds_ = k2 * _mm64(j_s.T, j_s) / n_s
        gs_ = -k2 * (j_s.T @ rr_s) / n_s
        fh_s, fb_s, nf_s = _flip_allowance(j_s, j_s2, rr_s, k2 / n_s)
    else:
        sdf_loss, ds_, gs_, fh_s, fb_s, nf_s = 0.0, np.zeros((n_unk, n_unk)), np.zeros(n_unk), np.zeros((n_unk, n_unk)), np.zeros(n_unk), 0
    if n_k:
        render_loss = float(np.mean(rr_r * rr_r))
        dr_ = k1 * _mm64(j_r.T, j_r) / n_k
        gr_ = -k1 * (j_r.T @ rr_r) / n_k
        fh_r, fb_r, nf_r = _flip_allowance(j_r, j_r2, rr_r, k1 / n_k)
    else:
        render_loss, dr_, gr_, fh_r, fb_r, nf_r = 0.0, np.zeros((n_unk, n_unk)), np.zeros(n_unk), np.zeros((n_unk, n_unk)), np.zeros(n_unk), 0
    h_code = np.zeros((n_unk, n_unk))
    h_code[pd:, pd:] = k3 * np.eye(c_len)
    b_code = np.zeros(n_unk)
    b_code[pd:] = -k3 * z
    h_rot = np.zeros((n_unk, n_unk))
    h_rot[:pd, :pd] = k4 * np.outer(j_rot, j_rot)
    b_rot = np.zeros(n_unk)
    b_rot[:pd] = k4 * j_rot * res_rot
    h_damp = np.zeros((n_unk, n_unk))
    h_damp[:pd, :pd] = np.eye(pd)
    h_damp[pd - 1, pd - 1] += float(F32(prm.s_damp))
    h = dr_ + ds_ + h_code + h_rot + h_damp
    b = gr_ + gs_ + b_code + b_rot
    return dict(H=h, b=b, dx=np.linalg.solve(h, b), Dr=dr_, Ds=ds_, gr=gr_, gs=gs_, Lr=k1 * render_loss, Ls=k2 * sdf_loss,
                H_code_prior=h_code, b_code_prior=b_code, H_rot=h_rot, b_rot=b_rot, j_rot=j_rot, res_rot=res_rot, H_damp=h_damp,
                H_flip=fh_s + fh_r, b_flip=fb_s + fb_r, n_flip=(nf_s, nf_r),
                V=int(sum(r["V"] for r in rows)), K=int(n_k), N=int(n_s), loss=k1 * render_loss + k2 * sdf_loss)


def linearise_fp64(dec, prm, pts, rays, depth, t_obj_cam, code, depths, sets):
    """One Gauss-Newton system of reconstruct_object (optimizer.py:129-186) evaluated in float64 throughout, at the state
    (t_obj_cam, code) with the depth samples `depths`, on the sample sets the caller decided: sets = the fp32 trace's `sets`
    (`valid` = in-sphere (ray, depth) indices, `kept` = rendered rows).  No threshold is re-applied here -- fp64 and fp32 may
    decide a sample within round-off of a threshold differently, and the comparison is of arithmetic on one set.

    Returns a dict: H, b, dx (the system and its solve), Dr / Ds (data Grams k1 J_r^T J_r / K and k2 J_s^T J_s / N, no prior, no
    damping), gr / gs (data parts of b: -k1 J_r^T r_r / K, -k2 J_s^T r_s / N), Lr / Ls (k1 render_loss, k2 sdf_loss), the prior
    terms H_code_prior (k3), b_code_prior (-k3 z), H_rot / b_rot (the k4 rotation prior as added to H and b), j_rot, H_damp (the
    pose-block damping), V, K, N, loss.  H_flip / b_flip: what the surface and render rows with a hidden ReLU within round-off of its
    kink (RELU_ULPS) would change in H and b, entry by entry, on the other side of it -- an fp32 implementation may land on either side,
    and the gradient jumps there (n_flip = the number of such surface and render rows).
    The rows come from _view_rows64 and are put together by _assemble64, which linearise_fp64_multiview shares."""
    return _assemble64(prm, [_view_rows64(dec, prm, pts, rays, depth, t_obj_cam, code, depths, sets)], t_obj_cam, code)


NO_SETS = dict(valid=(np.zeros(0, np.int64), np.zeros(0, np.int64)), kept=(np.zeros(0, np.int64), np.zeros(0, np.int64)))


def view_matrix(t_obj_cam, t_ref_cam):
    """T_oc_v = T_oc T_ref_v: the fp64 product of the two fp32 matrices, rounded once to fp32."""
    return (np.asarray(t_obj_cam, F32).astype(F64) @ np.asarray(t_ref_cam, F32).astype(F64)).astype(F32)


def linearise_fp64_multiview(dec, prm, views, t_obj_cam, code, depths_per_view, sets_per_view, rows_out=None):
    """linearise_fp64 for one object seen by several cameras: views = [dict(t_ref_cam, pts, rays, depth), ...]; view v's rows are
    linearise_fp64's rows at view_matrix(t_obj_cam, t_ref_cam_v) on depths_per_view[v] and sets_per_view[v] (None, or empty `kept`: the
    view has no render rows), and the rows of all views are pooled as one row set -- divided by the pooled N and K -- while the priors
    and the damping are taken once at t_obj_cam.  Returns linearise_fp64's keys (V, K, N pooled) plus V_views / K_views / N_views.
    rows_out (optional list) receives each view's rows (_view_rows64)."""
    rows = []
    for v, d, s in zip(views, depths_per_view, sets_per_view):
        rows.append(_view_rows64(dec, prm, v["pts"], v["rays"], v["depth"], view_matrix(t_obj_cam, v["t_ref_cam"]), code, d, NO_SETS if s is None else s))
    if rows_out is not None:
        rows_out.extend(rows)
    lin = _assemble64(prm, rows, t_obj_cam, code)
    lin.update(V_views=[r["V"] for r in rows], K_views=[r["K"] for r in rows], N_views=[r["N"] for r in rows])
    return lin


def pose_only_system(dec, pts, t_obj_cam, code):
    """One pose-only linearisation (optimizer.py:62-72) at a camera->object matrix: dict(H (6,6), b (6,), dx (6,), res (N,), n).
    N = 0 gives what the reference computes for it: 0 / 0 = NaN in H and b, hence in dx."""
    j7, _, res = compute_sdf_loss(dec, np.asarray(pts, F32), np.asarray(t_obj_cam, F32), np.asarray(code, F32))
    j6 = j7[:, :6]
    n = F32(j6.shape[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        hess = ((j6.T @ j6) / n).astype(F32) + F32(1e-2) * np.eye(6, dtype=F32)   # :69-70
        b = (-(j6.T @ res) / n).astype(F32)                                       # :71 raw residual
    dx = (_inv(hess) @ b).astype(F32) if np.all(np.isfinite(hess)) else np.full(6, np.nan, F32)
    return dict(H=hess, b=b, dx=dx, res=np.asarray(res, F32).reshape(-1), n=int(j6.shape[0]))


POSE_INLIER_TH = F32(0.05)     # optimizer.py:77


def estimate_pose_cam_obj(dec, prm, t_co_se3, scale, pts, code, trace=None, states=None):
    """Optimizer.estimate_pose_cam_obj (optimizer.py:45-86) -> (4,4) f32 SE(3) object->camera.

    (The reference scales the caller's array in place, :53-54; this restatement works on a copy.)
    trace (optional list) receives one dict per iteration: the state it started from, H, b, dx, n = the number of points its system was
    built from, and at e == 4 the residual `res` and the inlier mask `mask` that the filter of :76-78 keeps for the following iterations.
    An object without points (from the start, or after the filter) gives NaN everywhere, as in the reference.
    states (tests only): iteration e linearises at states[e] -- a recorded camera->object matrix of the reference -- instead of where
    the previous update led.
    """
    t_cam_obj = np.asarray(t_co_se3, F32).copy()
    t_cam_obj[:3, :3] *= F32(scale)
    t_obj_cam = _inv(t_cam_obj)
    z = np.asarray(code, F32)
    pts = np.asarray(pts, F32).reshape(-1, 3)
    for e in range(prm.num_iterations_pose_only):
        if states is not None:
            t_obj_cam = np.asarray(states[e], F32).copy()
        it = pose_only_system(dec, pts, t_obj_cam, z)
        rec = dict(H=it["H"].copy(), b=it["b"].copy(), dx=it["dx"].copy(), t_obj_cam=t_obj_cam.copy(), n=it["n"])
        with np.errstate(invalid="ignore"):
            t_obj_cam = (exp_se3(it["dx"]) @ t_obj_cam).astype(F32)                # :73-74
        if e == 4:                                                                # :76-78: the residual from BEFORE this iteration's update
            keep = np.abs(it["res"]) <= POSE_INLIER_TH
            pts = pts[keep]
            rec.update(res=it["res"].copy(), mask=keep)
        if trace is not None:
            trace.append(rec)
    if not np.all(np.isfinite(t_obj_cam)):
        return np.full((4, 4), np.nan, F32)         # torch.inverse of a NaN matrix: NaN throughout
    out = _inv(t_obj_cam)
    out[:3, :3] /= F32(scale)
    return out
