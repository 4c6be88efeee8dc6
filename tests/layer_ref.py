"""The layers between the convs, restated in numpy float64 (no torch here): norm forward and backward, the four activations, MaxPool3d(2, 2),
nearest x2 upsample, views and their concatenation, the fp32-NCDHW export and the gradient import.

Layouts are the engine's: a norm tensor is [S][C] (voxels, channels), a volume [D][H][W][C]; exported tensors are [C][S].  A view is
act(x * scale[c] + shift[c]).  Conventions at 0 (unet-studio_amd/csrc/device_util.h act_d): relu' = 0, leaky' = 0.01, elu' = exp(0) = 1.
tests/test_layer_ref_host.py holds these against torch's float64 autograd and the C oracle; tests/test_gpu_layer_ops.py holds the
kernels of csrc/kernels_elem.hip against these."""
import numpy as np

MOMENTUM = 0.1
EPS = {"in": 1e-5, "bn": 0.0, "bn_eval": 0.0}     # graph.cpp: InstanceNorm 1e-5, BatchNorm 0


def act(z, a):
    z = np.asarray(z, np.float64)
    if a == 1:
        return np.where(z > 0, z, 0.0 * z)          # 0 * z keeps a NaN
    if a == 2:
        return np.where(z > 0, z, 0.01 * z)
    if a == 3:
        return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))
    return z


def act_d(z, a):
    z = np.asarray(z, np.float64)
    if a == 1:
        return np.where(z > 0, 1.0, 0.0)
    if a == 2:
        return np.where(z > 0, 1.0, 0.01)
    if a == 3:
        return np.where(z > 0, 1.0, np.exp(np.minimum(z, 0.0)))
    return np.ones_like(z)


def view(x, scale=None, shift=None, a=0):
    """what a consumer sees of a source: act(x * scale[c] + shift[c]), channels last"""
    x = np.asarray(x, np.float64)
    return act(x if scale is None else x * scale + shift, a)


def norm_fwd(u, gamma, beta, eps, rm=None, rv=None, use_running=False, keep=None):
    """u [S][C] -> mean, var (biased), rstd, scale = gamma rstd, shift = beta - mean scale, and the running statistics after the call
    (momentum 0.1, unbiased variance; unchanged in eval mode).  keep: the voxels the sums see (the divisor stays S: a wrong reference)"""
    u = np.asarray(u, np.float64)
    S = u.shape[0]
    out = {}
    if use_running:
        mean, var = np.asarray(rm, np.float64), np.asarray(rv, np.float64)
        out["rm"], out["rv"] = mean.copy(), var.copy()
    else:
        if keep is None:
            mean = u.sum(0) / S
            var = ((u - mean) ** 2).sum(0) / S
        else:
            mean = u[keep].sum(0) / S
            var = np.maximum((u[keep] ** 2).sum(0) / S - mean * mean, 0.0)
        if rm is not None:
            out["rm"] = (1 - MOMENTUM) * rm + MOMENTUM * mean
            out["rv"] = (1 - MOMENTUM) * rv + MOMENTUM * (var * S / (S - 1.0) if S > 1 else var)
    rstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * rstd
    out.update(mean=mean, var=var, rstd=rstd, scale=scale, shift=beta - mean * scale)
    return out


def norm_bwd(g, u, mean, rstd, scale, shift, gamma, a, keep=None):
    """g = dL/d(view of u) [S][C], the stat row as the kernel is given it -> dv = g act'(u scale + shift), xhat, coef = {c0 = gamma rstd,
    m1 = mean(dv), m2 = mean(dv xhat)}, dgamma = sum dv xhat, dbeta = sum dv, du = c0 (dv - m1 - xhat m2) = dL/d(raw u).
    keep: the voxels the sums see (a wrong reference)"""
    g, u = np.asarray(g, np.float64), np.asarray(u, np.float64)
    S = u.shape[0]
    z = u * scale + shift
    ad = act_d(z, a)
    dv = g * ad
    xhat = (u - mean) * rstd
    k = slice(None) if keep is None else keep
    dbeta, dgamma = dv[k].sum(0), (dv[k] * xhat[k]).sum(0)
    c0, m1, m2 = gamma * rstd, dbeta / S, dgamma / S
    return dict(z=z, ad=ad, dv=dv, xhat=xhat, c0=c0, m1=m1, m2=m2, dgamma=dgamma, dbeta=dbeta, du=c0 * (dv - m1 - xhat * m2))


def _windows(x):
    """[D][H][W][C] -> [Do][Ho][Wo][8][C], window element t = (dz << 2) | (dy << 1) | dx: the (z, y, x) scan order"""
    D, H, W, C = x.shape
    Do, Ho, Wo = D // 2, H // 2, W // 2
    w = x[:2 * Do, :2 * Ho, :2 * Wo].reshape(Do, 2, Ho, 2, Wo, 2, C)
    return w.transpose(0, 2, 4, 1, 3, 5, 6).reshape(Do, Ho, Wo, 8, C)


def maxpool_fwd(x):
    """MaxPool3d(2, 2), floor mode -> (y [Do][Ho][Wo][C], arg: the window element that holds it).  The first maximum in scan order
    wins; a NaN beats everything before it and only a later NaN beats a NaN, so the last NaN of a window wins"""
    w = _windows(np.asarray(x, np.float64))
    best = np.full(w.shape[:3] + w.shape[4:], -np.inf)
    arg = np.zeros(best.shape, np.int64)
    for t in range(8):
        v = w[:, :, :, t]
        with np.errstate(invalid="ignore"):
            take = (v > best) | np.isnan(v)
        best = np.where(take, v, best)
        arg = np.where(take, t, arg)
    return best, arg


def maxpool_bwd(gout, arg, shape, second=False, x=None):
    """dx [D][H][W][C]: gout at each window's arg, 0 elsewhere (the trailing plane of an odd extent too).  second (a wrong reference):
    a window whose maximum occurs twice sends its gradient to the second occurrence (x: the pooled tensor)"""
    D, H, W, C = shape
    Do, Ho, Wo = D // 2, H // 2, W // 2
    gout = np.asarray(gout, np.float64)
    if second:
        w = _windows(np.asarray(x, np.float64))
        best = np.take_along_axis(w, arg[:, :, :, None], 3)[:, :, :, 0]
        nxt = arg.copy()
        for t in range(7, -1, -1):      # ends at the lowest t above arg that holds the same value
            nxt = np.where((w[:, :, :, t] == best) & (t > arg), t, nxt)
        arg = nxt
    dxw = np.zeros((Do, Ho, Wo, 8, C))
    np.put_along_axis(dxw, arg[:, :, :, None], gout[:, :, :, None], 3)
    dx = np.zeros(shape)
    dx[:2 * Do, :2 * Ho, :2 * Wo] = dxw.reshape(Do, Ho, Wo, 2, 2, 2, C).transpose(0, 3, 1, 4, 2, 5, 6).reshape(2 * Do, 2 * Ho, 2 * Wo, C)
    return dx


def upsample_fwd(x):
    return np.repeat(np.repeat(np.repeat(np.asarray(x, np.float64), 2, 0), 2, 1), 2, 2)


def upsample_bwd(gout):
    g = np.asarray(gout, np.float64)
    D, H, W, C = g.shape[0] // 2, g.shape[1] // 2, g.shape[2] // 2, g.shape[3]
    return g.reshape(D, 2, H, 2, W, 2, C).sum((1, 3, 5))


def concat(views):
    return np.concatenate([np.asarray(v, np.float64) for v in views], -1)


def concat_bwd(gout, channels):
    """the slices of gout along the channel axis, one per source"""
    g = np.asarray(gout, np.float64)
    edges = np.cumsum([0] + list(channels))
    return [g[..., edges[i]:edges[i + 1]] for i in range(len(channels))]


def export(v):
    """a view [S][C] (or a volume, flattened) -> NCDHW [C][S]"""
    v = np.asarray(v, np.float64)
    return np.ascontiguousarray(v.reshape(-1, v.shape[-1]).T)


def import_grad(g, old=None):
    """NCDHW [C][S] -> [S][C], added to old where given"""
    r = np.ascontiguousarray(np.asarray(g, np.float64).T)
    return r if old is None else r + old
