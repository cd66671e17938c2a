"""Plain reference of the temporal transformer's attention core, written out from the formula, and of its dropout hash.
No project imports: the tests compare the HIP kernels (csrc/causal_attn.hip) with this file.

attention() is the operator chain  scale q k^T -> masked_fill -> softmax -> (* keep / (1 - p)) -> @ v  on token-major
rows (row l * B + b, head h in columns h * D .. h * D + D - 1) in the dtype and on the device of its inputs: float64
inputs give the reference (gradients: float64 autograd of this chain), float32 inputs give 'the f32 operator chain' that
the tests calibrate their bound with.  keep_mask() restates attn_keep in numpy uint32.  slice_error() is the error norm
of the tests: per (tracklet, head) slice, so that a wrong head with small values does not hide behind the largest one."""
import numpy as np
import torch


def heads(t, n, B, H, D):
    """[n B, H D] token-major -> [B H, n, D]"""
    return t.reshape(n, B * H, D).transpose(0, 1)


def combined_mask(B, H, L, S, attn_mask, key_pad):
    """bool [B, H, L, S], True = not allowed; None without any mask"""
    m = None
    if attn_mask is not None:
        m = attn_mask.bool()[None, None].expand(B, H, L, S)
    if key_pad is not None:
        kp = key_pad.bool()[:, None, None, :].expand(B, H, L, S)
        m = kp if m is None else m | kp
    return m


def probabilities(q, k, dims, attn_mask, key_pad):
    """[B H, L, S] softmax(mask(scale q k^T)), before dropout"""
    B, H, L, S, D = dims
    scores = torch.bmm(heads(q, L, B, H, D) * D ** -0.5, heads(k, S, B, H, D).transpose(1, 2))
    m = combined_mask(B, H, L, S, attn_mask, key_pad)
    if m is not None:
        scores = scores.masked_fill(m.reshape(B * H, L, S).to(scores.device), float('-inf'))
    return torch.softmax(scores, -1)


def attention(q, k, v, dims, attn_mask, key_pad, keep=None, p=0.0):
    """q [L B, H D], k / v [S B, H D] -> [L B, H D].  attn_mask bool [L, S], key_pad bool [B, S] (True = not allowed) or
    None; keep: [B H, L, S] of the elements the dropout keeps (any dtype; None: no dropout), p its probability."""
    B, H, L, S, D = dims
    prob = probabilities(q, k, dims, attn_mask, key_pad)
    if keep is not None:
        prob = prob * torch.as_tensor(keep).to(device=prob.device, dtype=prob.dtype) / (1.0 - p)
    return torch.bmm(prob, heads(v, S, B, H, D)).transpose(0, 1).reshape(L * B, H * D)


def drop_threshold(p):
    """an element is kept when its 24-bit hash >= this (the C entry points: (uint32_t)(p * 16777216.f), p a float)"""
    return np.uint32(np.float32(p) * np.float32(16777216.0))


def keep_mask(seed, BH, L, S, p):
    """bool [BH, L, S]: the elements attn_keep keeps.  One 32-bit hash of (element index, seed) per element, its upper
    24 bits against the threshold.  uint32 arithmetic (wrapping)."""
    u32 = np.uint32
    thr = drop_threshold(p)
    if thr == 0:
        return np.ones((BH, L, S), dtype=bool)
    seed = int(seed) & (2 ** 64 - 1)
    lo, hi = u32(seed & 0xffffffff), u32(seed >> 32)
    assert BH * L * S < 2 ** 31
    with np.errstate(over='ignore'):
        h = np.arange(BH * L * S, dtype=u32) ^ lo      # element (bh * L + l) * S + s
        h = h * u32(0x9E3779B1)
        h = h ^ (h >> u32(16))
        h = (h + hi) * u32(0x85EBCA6B)
        h = h ^ (h >> u32(13))
        h = h * u32(0xC2B2AE35)
        h = h ^ (h >> u32(16))
    return ((h >> u32(8)) >= thr).reshape(BH, L, S)


def slice_error(got, ref, B, H, D):
    """got, ref: token-major [n B, H D].  -> (rel, zero_abs): rel = max over the (tracklet, head) slices whose reference is
    not identically zero of max|got - ref| / max|ref| of that slice; zero_abs = max|got - ref| over the slices whose
    reference IS identically zero (0.0 when there is none) -- those have no scale of their own, the caller bounds them
    absolutely.  A NaN in got makes the result NaN (which fails every <=)."""
    n = ref.shape[0] // B
    g = got.detach().to(device=ref.device, dtype=torch.float64).reshape(n, B, H, D)
    r = ref.detach().to(torch.float64).reshape(n, B, H, D)
    err = (g - r).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err).amax(dim=(0, 3))    # [B, H]
    top = r.abs().amax(dim=(0, 3))
    zero = top == 0
    rel = torch.where(zero, torch.zeros_like(err), err / top.clamp_min(1e-300))
    rel, zero_abs = float(rel.max()), float(torch.where(zero, err, torch.zeros_like(err)).max())
    nan = float('nan')
    return (nan if rel == float('inf') else rel), (nan if zero_abs == float('inf') else zero_abs)
