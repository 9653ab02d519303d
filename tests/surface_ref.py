"""Surface projection (include/dsp_gn.h dsp_surface_points): the statements the tests hold the library to.

* step64 / attributes64 / refine64: the rule in numpy float64 on the fp64 oracle's decoder output (oracle.dsp_oracle._decode64), including
  its gradient on the other side of every ReLU kink within fp32 round-off of zero.
* step32 / attributes32: csrc/surface_math.h restated in numpy float32, one correctly rounded operation at a time in the header's order
  (numpy never contracts a multiply and an add), the 64-term sum in the header's tree -- what the host functions and the device must equal
  bit for bit.
"""
import numpy as np

TINY = 1e-20
F32 = np.float32


# ---- float64 ----------------------------------------------------------------------------------------------------------------------------
def step64(p, sdf, g, max_step):
    p, sdf, g = np.asarray(p, np.float64), np.asarray(sdf, np.float64), np.asarray(g, np.float64)
    g2 = (g * g).sum(1)
    with np.errstate(all="ignore"):
        d = (sdf / np.maximum(g2, TINY))[:, None] * g
        n = np.sqrt((d * d).sum(1))
        d = np.where((n > max_step)[:, None], d * (max_step / n)[:, None], d)
    move = (g2 >= TINY) & np.isfinite(d).all(1)
    return np.where(move[:, None], p - d, p)


def attributes64(grad, sdf, var=None):
    """grad (n, C + 3) = d sdf / d [code, xyz] -> normal (n, 3), |g| (n,), sdf, sigma (n,) or None."""
    grad = np.asarray(grad, np.float64)
    g = grad[:, -3:]
    gn = np.sqrt((g * g).sum(1))
    with np.errstate(all="ignore"):
        normal = np.where((gn * gn < TINY)[:, None], 0.0, g / gn[:, None])
        sigma = None
        if var is not None:
            c = grad.shape[1] - 3
            sigma = np.where(gn * gn < TINY, 0.0, np.sqrt((grad[:, :c] ** 2 * np.asarray(var, np.float64)[:c]).sum(1)) / gn)
    return normal, gn, np.asarray(sdf, np.float64), sigma


def decode64(dec, code, p, grad=True):
    """oracle: sdf (n,), gradient (n, C + 3), gradient on the other side of the near-zero ReLUs (both None without grad); dp = one fp32
    ulp of each coordinate."""
    from oracle import dsp_oracle as O
    p = np.asarray(p, np.float64)
    dp = np.abs(p) * 2.0 ** -24
    return O._decode64(dec, np.asarray(code, np.float64)[:dec.code_len], p, grad=grad, dp=dp)


def refine64(dec, code, p0, steps, max_step):
    """The projection in float64 from p0: (final points, |sdf| there (n,))."""
    p = np.asarray(p0, np.float64)
    for _ in range(steps):
        y, g, _ = decode64(dec, code, p)
        p = step64(p, y, g[:, -3:], max_step)
    y, _, _ = decode64(dec, code, p, grad=False)
    return p, np.abs(y)


# ---- float32, operation by operation ----------------------------------------------------------------------------------------------------
def _norm2_32(v):
    return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


def step32(p, sdf, g, max_step):
    p, sdf, g = np.asarray(p, F32).reshape(-1, 3), np.asarray(sdf, F32).reshape(-1), np.asarray(g, F32).reshape(-1, 3)
    ms = F32(max_step)
    with np.errstate(all="ignore"):
        g2 = _norm2_32(g)
        move = (g2 >= F32(TINY)) & np.isfinite(g2)
        k = sdf / g2
        d = k[:, None] * g
        d2 = _norm2_32(d)
        s = ms / np.sqrt(d2)
        d = np.where((d2 > ms * ms)[:, None], s[:, None] * d, d)
        move &= np.isfinite(d).all(1)
        out = np.where(move[:, None], p - d, p)
    assert out.dtype == F32
    return out


def tree_sum32(terms):
    """(n, 64) float32 -> (n,): 16 lanes x 4 entries left to right, then the xor butterfly with masks 1, 2, 4, 8; lane 0."""
    t = np.asarray(terms, F32).reshape(-1, 16, 4)
    s = ((t[:, :, 0] + t[:, :, 1]) + t[:, :, 2]) + t[:, :, 3]
    lanes = np.arange(16)
    for m in (1, 2, 4, 8):
        s = s + s[:, lanes ^ m]
    assert s.dtype == F32
    return s[:, 0]


def attributes32(rows68, var=None):
    """rows (n, 68) float32, var 64 values or None -> normal, grad_norm, sdf, sigma (or None), all float32."""
    r = np.asarray(rows68, F32).reshape(-1, 68)
    g = r[:, 64:67]
    with np.errstate(all="ignore"):
        g2 = _norm2_32(g)
        gn = np.sqrt(g2)
        flat = g2 < F32(TINY)
        normal = np.where(flat[:, None], F32(0), g / gn[:, None])
        sigma = None
        if var is not None:
            v = np.asarray(var, np.float64).astype(F32)
            S = tree_sum32((r[:, :64] * r[:, :64]) * v[None, :])
            sigma = np.where(flat, F32(0), np.sqrt(S) / gn)
    return normal.astype(F32), gn, r[:, 67].copy(), sigma


def rows68(sdf, grad67):
    """dsp_sdf_jacobian's outputs (sdf (n,), grad (n, 67)) as the 68-float rows the decoder kernel writes."""
    return np.ascontiguousarray(np.concatenate([np.asarray(grad67, F32), np.asarray(sdf, F32)[:, None]], 1))
