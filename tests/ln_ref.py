"""Plain float64 reference of LayerNorm (+ exact-erf GELU, + the folded dropout) over feature rows, written out from the
formulas: forward, backward without autograd, and the keep mask of the dropout hash.  No project imports: the tests
compare the HIP kernels (csrc/layernorm_act.hip, csrc/ln_math.hpp) with this file.  The tensor functions run on
whatever device their inputs are on (CPU for the small cases, the GPU's float64 units for the large ones)."""
import math

import numpy as np
import torch


def _gelu_on(act):
    return act in (1, 'gelu')


def _f64(t, like=None):
    t = torch.as_tensor(t)
    return t.to(device=t.device if like is None else like.device, dtype=torch.float64)


def norm_cdf(z):
    """Phi(z) through erfc, so that the lower tail keeps its relative accuracy"""
    return 0.5 * torch.erfc(-z * math.sqrt(0.5))


def gelu(z):
    return z * norm_cdf(z)


def gelu_grad(z):
    """d GELU / dz = Phi(z) + z phi(z)"""
    return norm_cdf(z) + z * torch.exp(-0.5 * z * z) * (1.0 / math.sqrt(2.0 * math.pi))


def row_stats(x, eps):
    x = _f64(x)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return mean, 1.0 / torch.sqrt(var + float(eps))


def ln_act(x, gamma, beta, eps, act, keep=None, scale=1.0):
    """-> y [n, c], mean [n], rstd [n] in float64.  keep: bool [n, c] of the elements the dropout keeps (scaled by
    `scale`), None for no dropout."""
    x = _f64(x)
    gamma, beta = _f64(gamma, x), _f64(beta, x)
    mean, rstd = row_stats(x, eps)
    z = (x - mean[:, None]) * rstd[:, None] * gamma + beta
    y = gelu(z) if _gelu_on(act) else z
    if keep is not None:
        y = y * (torch.as_tensor(keep).to(x.device).to(torch.float64) * float(scale))
    return y, mean, rstd


def ln_act_backward_terms(x, dy, gamma, beta, eps, act, keep=None, scale=1.0, stats=None):
    """Every intermediate of the backward as a dict (float64).  stats = (mean, rstd) replaces the row statistics of x:
    the backward kernels READ the stored statistics, so a test that hands them given numbers states the same here."""
    x, dy = _f64(x), _f64(dy)
    gamma, beta = _f64(gamma, x), _f64(beta, x)
    mean, rstd = row_stats(x, eps) if stats is None else (_f64(stats[0], x), _f64(stats[1], x))
    c = x.shape[1]
    if keep is not None:   # the forward multiplied by keep * scale behind the activation
        dy = dy * (torch.as_tensor(keep).to(x.device).to(torch.float64) * float(scale))
    xhat = (x - mean[:, None]) * rstd[:, None]
    z = xhat * gamma + beta
    dz = dy * gelu_grad(z) if _gelu_on(act) else dy
    dzg = dz * gamma
    s1 = dzg.sum(1, keepdim=True) / c
    s2 = (dzg * xhat).sum(1, keepdim=True) / c
    dx = rstd[:, None] * (dzg - s1 - xhat * s2)
    return dict(dx=dx, dgamma=(dz * xhat).sum(0), dbeta=dz.sum(0), abs_dgamma=(dz * xhat).abs().sum(0),
                abs_dbeta=dz.abs().sum(0), dy=dy, xhat=xhat, z=z, dz=dz, dzg=dzg, s1=s1, s2=s2, mean=mean, rstd=rstd)


def ln_act_backward(x, dy, gamma, beta, eps, act, keep=None, scale=1.0, stats=None):
    """-> dx [n, c], dgamma [c], dbeta [c], sum_rows |dz * xhat| [c], sum_rows |dz| [c]  (the last two: what a bound on
    the summation error of dgamma / dbeta scales with)"""
    t = ln_act_backward_terms(x, dy, gamma, beta, eps, act, keep, scale, stats)
    return t['dx'], t['dgamma'], t['dbeta'], t['abs_dgamma'], t['abs_dbeta']


def dropout_keep(n, c, thr, seed):
    """bool [n, c]: the elements ln_dropout_mask2 keeps.  One 32-bit hash per channel pair of (row, pair, seed), the
    even channel against its low 16 bits, the odd one against its high 16 bits.  uint32 arithmetic (wrapping)."""
    assert c % 2 == 0 and 0 <= thr < 65536
    u32 = np.uint32
    seed = int(seed) & (2 ** 64 - 1)
    seed_lo, seed_hi = u32(seed & 0xffffffff), u32(seed >> 32)
    row64 = np.arange(n, dtype=np.int64)[:, None]
    row = (row64 & 0xffffffff).astype(u32)
    pair = np.arange(c // 2, dtype=u32)[None, :]
    h = (row * u32(c // 2) + pair) ^ seed_lo
    h = h * u32(0x9E3779B1)
    h = h ^ (h >> u32(16))
    h = (h + seed_hi + (row64 >> 24).astype(u32)) * u32(0x85EBCA6B)
    h = h ^ (h >> u32(13))
    h = h * u32(0xC2B2AE35)
    h = h ^ (h >> u32(16))
    keep = np.empty((n, c), dtype=bool)
    keep[:, 0::2] = (h & u32(0xffff)) >= u32(thr)
    keep[:, 1::2] = (h >> u32(16)) >= u32(thr)
    return keep
