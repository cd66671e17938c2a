"""The attention core of the temporal transformer (csrc/causal_attn.hip, ococc_temporal_attention_{fwd,bwd}_f32,
occ/layers.py:_TemporalAttention) against the float64 chain of tests/attn_ref.py where its code takes another path or a
number format ends: L != S (the two workgroup roles of the backward launch index their LDS rows by l and by s), the tile
and chunk edges (16 rows per workgroup, 64 staged rows per chunk), L = S = 256 and D = 384 (the largest LDS request),
head widths that are no multiple of 64, D = 4, a single query, a single key, all four mask kinds, operands that are column
slices of wider buffers (NaN in the gaps, sentinels around the outputs), peaked / uniform / shifted / underflowing
logits, a fully masked tracklet, the dropout hash against its numpy restatement for seeds that differ in either word,
the host-seed arguments, determinism, the refusals and the module with key is not query.

The accuracy bound, the same for every numeric case: with slice_error = max over the (tracklet, head) slices of
max|got - ref| / max|ref| of that slice (ref: the float64 chain),

    slice_error(kernel) <= 4 * slice_error(f32 operator chain on the GPU, same inputs) + 8 * 2^-24

for out, dq, dk and dv.  The baseline is the operator chain's own float32 arithmetic, never the kernel: 4 covers another
summation order and __expf (about 2 ulp, plus an argument error of |x - m| 2^-24 on the terms that matter), the additive
term the cases where the chain happens to be exact.  Slices whose reference is identically zero (dq / dk when one key is
left: the kernel computes p (dO . v - dO . O), which cancels to rounding only) are bounded absolutely by
4 D 2^-24 max|dO| max|v| max(|q|, |k|) / sqrt(D): D products of at most max|dO| max|v|, each off by 2^-24 in either of the
two dot products, times the q or k row and the scale that the gradient is multiplied with; 4 for the two sums and the
order.  out and dv have no such slices short of a probability that is exactly 0, which the kernel multiplies through:
theirs must be exactly 0.  Rows of dk and dv of padded keys must be exactly 0.0.

Each case prints one line 'ATTNEDGE <case>: out a/b dq a/b dk a/b dv a/b', a = slice_error(kernel) / slice_error(chain)
and b = slice_error(kernel) / bound (pytest -s shows them).  Measured on gfx950 when this file was written:

    case                               out        dq         dk         dv
    2x2x65x130x64 none                 0.71/0.15  0.99/0.22  0.58/0.13  0.71/0.15
    2x2x65x130x64 future               0.90/0.18  0.59/0.13  0.85/0.18  0.94/0.19
    2x2x65x130x64 future+padding       0.69/0.14  0.71/0.15  0.75/0.15  0.87/0.18
    2x2x65x130x64 random               1.24/0.25  1.32/0.27  0.88/0.17  0.73/0.15
    2x2x130x65x64 none                 0.56/0.12  0.64/0.14  0.70/0.15  0.69/0.15
    2x2x130x65x64 future               0.73/0.12  1.27/0.23  1.32/0.26  1.13/0.24
    2x2x130x65x64 future+padding       0.58/0.11  0.63/0.12  1.14/0.22  1.00/0.21
    2x2x130x65x64 random               0.83/0.16  0.68/0.13  0.78/0.16  0.84/0.16
    2x2x16x64x32 future                0.62/0.12  0.70/0.14  0.46/0.10  0.84/0.16
    2x2x16x64x32 random                1.01/0.17  0.82/0.15  1.14/0.19  0.67/0.12
    2x2x17x65x32 none                  0.50/0.11  1.68/0.30  0.88/0.18  0.60/0.12
    2x2x17x65x32 future+padding        0.41/0.08  0.62/0.12  0.33/0.07  0.35/0.07
    2x2x15x63x36 future                0.71/0.14  0.71/0.14  1.33/0.24  0.68/0.13
    2x2x15x63x36 random                1.07/0.19  1.00/0.17  1.03/0.18  0.93/0.17
    1x1x256x256x384 none               0.47/0.11  0.52/0.12  0.52/0.12  0.59/0.13
    1x1x256x256x384 future             0.48/0.09  0.57/0.13  0.64/0.14  0.87/0.19
    1x1x256x256x384 random             0.36/0.08  0.47/0.11  0.54/0.12  0.26/0.06
    1x2x255x256x380 future             0.66/0.14  0.42/0.10  0.90/0.20  0.92/0.20
    1x2x255x256x380 random             0.52/0.12  0.44/0.10  0.31/0.07  0.43/0.10
    3x1x1x256x4 none                   1.81/0.28  1.46/0.25  0.66/0.11  1.11/0.15
    3x1x1x256x4 future+padding         0.93/0.15  1.72/0.33  1.21/0.13  1.34/0.20
    3x1x1x256x4 random                 1.38/0.23  3.23/0.45  0.94/0.15  0.71/0.11
    2x1x256x1x4 none                   0.00/0.00  0.00/0.00  0.00/0.00  4.05/0.63
    2x1x256x1x4 future                 0.00/0.00  0.00/0.00  0.00/0.00  2.25/0.36
    33x4x32x32x384 none                0.44/0.10  0.60/0.14  0.69/0.16  0.62/0.14
    33x4x32x32x384 future              0.64/0.14  0.95/0.22  1.22/0.27  0.83/0.17
    33x4x32x32x384 future+padding      0.56/0.12  1.33/0.30  1.41/0.31  0.79/0.17
    2x2x200x200x128 peaked x12         0.40/0.10  0.36/0.09  0.46/0.11  0.52/0.12
    2x2x96x96x380 peaked x12           0.46/0.11  0.46/0.11  0.37/0.09  0.36/0.09
    2x2x200x200x128 peaked x40         0.95/0.23  0.38/0.09  0.29/0.07  1.02/0.25
    2x2x96x96x380 peaked x40           0.42/0.10  0.38/0.09  0.41/0.10  0.66/0.16
    2x2x200x200x128 uniform            0.99/0.08  0.74/0.14  0.00/0.00  1.00/0.22
    2x2x96x96x380 uniform              1.07/0.08  0.74/0.15  0.00/0.00  1.00/0.20
    2x2x200x200x128 shifted +300       0.49/0.12  0.59/0.15  0.38/0.09  0.50/0.12
    2x2x96x96x380 shifted +300         0.50/0.13  0.49/0.12  0.56/0.14  0.35/0.09
    2x2x200x200x128 underflow          0.56/0.14  0.51/0.13  0.40/0.10  0.45/0.11
    2x2x96x96x380 underflow            0.57/0.14  0.36/0.09  0.41/0.10  0.58/0.14
    2x2x200x200x128 tracklet 1 masked  0.41/0.08  -          -          -
    2x2x96x96x380 tracklet 1 masked    0.42/0.09  -          -          -
    2x2x200x200x384 dropout 0.1        0.59/0.12  0.98/0.21  0.98/0.21  0.78/0.16
    3x2x70x130x132 dropout 0.5         0.42/0.10  0.81/0.18  0.64/0.14  0.49/0.11
    2x4x32x32x64 dropout 0.1           0.64/0.11  1.27/0.25  1.38/0.27  1.01/0.17

(0.00/0.00: kernel and chain both exact, or a reference that is zero throughout.)  The largest b is 0.63, the largest a 4.05
(dv with a single key, where the chain is within an ulp of exact and the additive term is what the bound consists of).
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R        # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = -7777.0
EUNSUPPORTED, EINVAL = -3, -1
SEED_A, SEED_B, SEED_C = 123456789, 123456789 + 2 ** 32, 2 ** 62 - 1


@pytest.fixture(scope='module')
def lib():
    from objectcentricocccompletion_amd import _lib
    return _lib


# ---- inputs ----------------------------------------------------------------------------------------------------------

def _inputs(dims, seed):
    """q [L B, E], k, v [S B, E], d_out [L B, E]: float32, unit variance, from a seeded CPU generator"""
    B, H, L, S, D = dims
    g = torch.Generator().manual_seed(seed)
    E = H * D
    return (torch.randn(L * B, E, generator=g), torch.randn(S * B, E, generator=g), torch.randn(S * B, E, generator=g),
            torch.randn(L * B, E, generator=g))


def _masks(kind, dims, seed):
    """-> attn_mask bool [L, S] or None, key_pad bool [B, S] or None (True = not allowed); every row keeps a key"""
    B, H, L, S, D = dims
    g = torch.Generator().manual_seed(seed + 77)
    future = torch.triu(torch.ones(L, S, dtype=torch.bool), 1 + max(0, S - L))
    if kind == 'none':
        return None, None
    if kind == 'future':
        return future, None
    if kind == 'future+padding':   # tracklet 0: nothing padded; tracklet 1: exactly one key left; the others: anything
        assert B >= 2
        lens = torch.randint(1, S + 1, (B,), generator=g)
        lens[0], lens[1] = S, 1
        return future, torch.arange(S)[None, :] >= lens[:, None]
    if kind == 'random':
        m = torch.rand(L, S, generator=g) < 0.5
        m[torch.arange(L), torch.randint(0, S, (L,), generator=g)] = False
        return m, None
    raise ValueError(kind)


def _u8(m, dev):
    return None if m is None else m.to(dev).contiguous().view(torch.uint8)


# ---- the kernel, two ways --------------------------------------------------------------------------------------------

def _apply(dev, dims, q, k, v, d_out, attn_mask, key_pad, p=0.0, seed=None, backward=True):
    """through the autograd function, as the module calls it.  q / k / v: device tensors (any row stride the kernel takes);
    k None: q is the packed q | k.  -> dict of out (, dq, dk, dv)"""
    from objectcentricocccompletion_amd.occ.layers import _TemporalAttention
    B, H, L, S, D = dims
    leaves = [t.detach().requires_grad_(backward) for t in (q, k, v) if t is not None]
    ql, kl, vl = leaves if k is not None else (leaves[0], None, leaves[1])
    seed_t = None if seed is None else torch.tensor([seed], dtype=torch.int64, device=dev)
    out = _TemporalAttention.apply(ql, kl, vl, _u8(attn_mask, dev), _u8(key_pad, dev), dims, p, seed_t)
    res = {'out': out.detach()}
    if backward:
        out.backward(d_out)
        if k is None:
            res.update(dq=ql.grad[:, :H * D], dk=ql.grad[:, H * D:], dv=vl.grad)
        else:
            res.update(dq=ql.grad, dk=kl.grad, dv=vl.grad)
    return res


def _framed(rows, E, pad, dev):
    """a sentinel-filled [rows, pad + E + pad] buffer and its payload columns"""
    buf = torch.full((rows, E + 2 * pad), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[:, pad:pad + E]


def _direct(lib, dev, dims, q, k, v, d_out, attn_mask, key_pad, p=0.0, seed=0, seed_on_device=True, pad=0, spare=0,
            backward=True, expect_rc=0):
    """the two exports called through _lib.  Outputs live in sentinel-filled buffers: `pad` extra columns on either side of
    every output row, `spare` floats behind probs.  -> dict with the payloads, the whole buffers ('*_buf') and the return
    codes."""
    B, H, L, S, D = dims
    E = H * D
    res = {}
    res['probs_buf'] = torch.full((B * H * L * S + spare,), SENTINEL, dtype=torch.float32, device=dev)
    res['out_buf'], res['out'] = _framed(L * B, E, pad, dev)
    am, kp = _u8(attn_mask, dev), _u8(key_pad, dev)
    seed_t = torch.tensor([seed], dtype=torch.int64, device=dev) if (seed_on_device and p > 0) else None
    host_seed = 0 if seed_on_device else seed
    scale = float(D) ** -0.5
    res['rc_fwd'] = lib.lib.ococc_temporal_attention_fwd_f32(
        q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), lib.ptr(am), lib.ptr(kp),
        B, H, L, S, D, scale, float(p), host_seed, lib.ptr(seed_t), res['probs_buf'].data_ptr(), res['out'].data_ptr(),
        res['out'].stride(0), lib.stream())
    assert res['rc_fwd'] == expect_rc, lib.lib.ococc_last_error().decode(errors='replace')
    res['probs'] = res['probs_buf'][:B * H * L * S].view(B * H, L, S)
    if backward:
        for name, rows in (('dq', L * B), ('dk', S * B), ('dv', S * B)):
            res[name + '_buf'], res[name] = _framed(rows, E, pad, dev)
        res['rc_bwd'] = lib.lib.ococc_temporal_attention_bwd_f32(
            q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), B, H, L, S, D, scale,
            float(p), host_seed, lib.ptr(seed_t), res['probs_buf'].data_ptr(), res['out'].data_ptr(), res['out'].stride(0),
            d_out.data_ptr(), d_out.stride(0), res['dq'].data_ptr(), res['dq'].stride(0), res['dk'].data_ptr(),
            res['dk'].stride(0), res['dv'].data_ptr(), res['dv'].stride(0), lib.stream())
        assert res['rc_bwd'] == expect_rc, lib.lib.ococc_last_error().decode(errors='replace')
    torch.cuda.synchronize()
    return res


# ---- the check -------------------------------------------------------------------------------------------------------

def _chain(q, k, v, d_out, dims, attn_mask, key_pad, keep, p, dtype, device, backward):
    """tests/attn_ref.py's chain and its autograd gradients in `dtype` on `device` -> dict of detached tensors"""
    leaves = [t.detach().to(device=device, dtype=dtype).requires_grad_(backward) for t in (q, k, v)]
    out = R.attention(*leaves, dims, attn_mask, key_pad, keep=keep, p=p)
    res = {'out': out.detach()}
    if backward:
        out.backward(d_out.to(device=device, dtype=dtype))
        res.update(dq=leaves[0].grad, dk=leaves[1].grad, dv=leaves[2].grad)
    return res


def _tracklets(t, B, keep_b):
    """the rows of the tracklets keep_b of a token-major [n B, E] tensor"""
    if keep_b is None:
        return t
    n = t.shape[0] // B
    return t.reshape(n, B, -1)[:, keep_b].reshape(n * len(keep_b), -1)


def _check(case, dev, dims, q, k, v, d_out, attn_mask, key_pad, got, keep=None, p=0.0, tracklets=None):
    """got: the kernel's out (and dq, dk, dv) for the CPU float32 inputs q, k, v, d_out.  Runs the f32 chain on the GPU
    and the float64 chain on the CPU on the same inputs and asserts the module's bound for every tensor in got.
    tracklets: compare these tracklets only (the others hold NaN by design)."""
    B, H, L, S, D = dims
    backward = 'dq' in got
    ref = _chain(q, k, v, d_out, dims, attn_mask, key_pad, keep, p, torch.float64, 'cpu', backward)
    f32 = _chain(q, k, v, d_out, dims, attn_mask, key_pad, keep, p, torch.float32, dev, backward)
    nB = B if tracklets is None else len(tracklets)
    top = lambda t: float(t.abs().max())
    zero_bound = 4 * D * U * top(d_out) * top(v) * max(top(q), top(k)) / math.sqrt(D)
    line, failures = [], []
    for name in ('out', 'dq', 'dk', 'dv') if backward else ('out',):
        r = _tracklets(ref[name], B, tracklets)
        assert bool(torch.isfinite(r).all()), f'{case} {name}: the reference is not finite'
        e_k, z_k = R.slice_error(_tracklets(got[name].cpu(), B, tracklets), r, nB, H, D)
        e_c, z_c = R.slice_error(_tracklets(f32[name].cpu(), B, tracklets), r, nB, H, D)
        bound = 4 * e_c + 8 * U
        ratio = e_k / e_c if e_c else (float('inf') if e_k else 0.0)
        line.append(f'{name} {ratio:.2f}/{e_k / bound:.2f}')
        if not e_k <= bound:
            failures.append(f'{name}: slice error {e_k:.3e} > 4 * {e_c:.3e} + 8 * 2^-24 = {bound:.3e}')
        z_bound = zero_bound if name in ('dq', 'dk') else 0.0
        if not z_k <= z_bound:
            failures.append(f'{name}: {z_k:.3e} in a slice whose reference is zero, bound {z_bound:.3e} (the chain: {z_c:.3e})')
    print(f'ATTNEDGE {case}: ' + ' '.join(line))
    assert not failures, f'{case}: ' + '; '.join(failures)
    if key_pad is not None and backward:
        padded = key_pad.T.reshape(-1)                     # row s * B + b
        if tracklets is not None:
            padded = _tracklets(padded[:, None], B, tracklets)[:, 0]
        for name in ('dk', 'dv'):
            rows = _tracklets(got[name].cpu(), B, tracklets)[padded]
            assert bool((rows == 0).all()), f'{case} {name}: a row of a padded key is not exactly 0'
    return ref


# ---- shapes and masks ------------------------------------------------------------------------------------------------

RECT_A, RECT_B, MAXSHAPE = (2, 2, 65, 130, 64), (2, 2, 130, 65, 64), (1, 1, 256, 256, 384)
CASES = [   # (B, H, L, S, D), mask kinds
    (RECT_A, ('none', 'future', 'future+padding', 'random')),          # rectangular, more than one chunk on either side
    (RECT_B, ('none', 'future', 'future+padding', 'random')),
    ((2, 2, 16, 64, 32), ('future', 'random')),                        # exact tiles
    ((2, 2, 17, 65, 32), ('none', 'future+padding')),                  # one past the tile and the chunk
    ((2, 2, 15, 63, 36), ('future', 'random')),                        # one short
    (MAXSHAPE, ('none', 'future', 'random')),                          # every limit at once
    ((1, 2, 255, 256, 380), ('future', 'random')),                     # ragged last column group, odd tail
    ((3, 1, 1, 256, 4), ('none', 'future+padding', 'random')),         # a single query, the narrowest head
    ((2, 1, 256, 1, 4), ('none', 'future')),                           # a single key
    ((33, 4, 32, 32, 384), ('none', 'future', 'future+padding')),      # the workload's layer shape, odd tracklet count
]


@pytest.mark.parametrize('dims,kind', [(d, m) for d, kinds in CASES for m in kinds],
                         ids=lambda x: 'x'.join(map(str, x)) if isinstance(x, tuple) else x)
def test_shapes_and_masks(dev, dims, kind):
    seed = sum(dims) * 10 + len(kind)
    q, k, v, d_out = _inputs(dims, seed)
    attn_mask, key_pad = _masks(kind, dims, seed)
    got = _apply(dev, dims, q.to(dev), k.to(dev), v.to(dev), d_out.to(dev), attn_mask, key_pad)
    _check(f'{"x".join(map(str, dims))} {kind}', dev, dims, q, k, v, d_out, attn_mask, key_pad, got)


# ---- layout ----------------------------------------------------------------------------------------------------------

def _same(a, b, what):
    assert torch.equal(a, b), f'{what}: not bit-identical ({int((a != b).sum())} elements differ)'


@pytest.mark.parametrize('dims,kind', [(RECT_A, 'future+padding'), (RECT_B, 'random'), (MAXSHAPE, 'future')],
                         ids=lambda x: 'x'.join(map(str, x)) if isinstance(x, tuple) else x)
def test_operands_in_wider_buffers_full_of_nan(dev, dims, kind):
    """q and k: separate column slices of one buffer, v: a slice of another (ldv != E), NaN everywhere else.  A load
    outside its slice shows in the result, which must be the contiguous operands' result bit for bit."""
    B, H, L, S, D = dims
    E, n = H * D, max(L, S) * B
    q, k, v, d_out = _inputs(dims, 31)
    attn_mask, key_pad = _masks(kind, dims, 31)
    plain = _apply(dev, dims, q.to(dev), k.to(dev), v.to(dev), d_out.to(dev), attn_mask, key_pad)
    wide = torch.full((n, 2 * E + 20), float('nan'), device=dev)
    qs, ks = wide[:L * B, 4:4 + E], wide[:S * B, E + 12:2 * E + 12]
    wide_v = torch.full((S * B, E + 12), float('nan'), device=dev)
    vs = wide_v[:, 8:8 + E]
    qs.copy_(q), ks.copy_(k), vs.copy_(v)
    assert vs.stride(0) != E and qs.stride(0) == ks.stride(0) != E
    got = _apply(dev, dims, qs, ks, vs, d_out.to(dev), attn_mask, key_pad)
    for name in ('out', 'dq', 'dk', 'dv'):
        assert bool(torch.isfinite(got[name]).all()), f'{name}: a NaN from outside the column slices'
        _same(got[name], plain[name], name)
    if L == S:   # the packed path: q | k handed over whole, itself a column slice of a NaN buffer
        packed = torch.full((L * B, 2 * E + 8), float('nan'), device=dev)
        qk = packed[:, 4:4 + 2 * E]
        qk[:, :E].copy_(q), qk[:, E:].copy_(k)
        got = _apply(dev, dims, qk, None, vs, d_out.to(dev), attn_mask, key_pad)
        for name in ('out', 'dq', 'dk', 'dv'):
            _same(got[name], plain[name], 'packed ' + name)


@pytest.mark.parametrize('dims,kind', [(RECT_A, 'future+padding'), (RECT_B, 'future+padding'), (MAXSHAPE, 'future')],
                         ids=lambda x: 'x'.join(map(str, x)) if isinstance(x, tuple) else x)
def test_outputs_stay_inside_their_columns(dev, lib, dims, kind):
    """out, dq, dk, dv with row strides wider than E and probs with spare floats behind it, all inside sentinel-filled
    allocations: the sentinels survive, the payload is _TemporalAttention's bit for bit (dropout on, so that the hash
    counter is part of it)."""
    B, H, L, S, D = dims
    q, k, v, d_out = (t.to(dev) for t in _inputs(dims, 32))
    attn_mask, key_pad = _masks(kind, dims, 32)
    p = 0.1
    E = H * D
    got = _direct(lib, dev, dims, q, k, v, d_out, attn_mask, key_pad, p=p, seed=SEED_B, pad=8, spare=64)
    for name in ('out', 'dq', 'dk', 'dv'):   # (first: a kernel that fails here must not go on to the tight buffers below)
        buf = got[name + '_buf']
        intact = bool((buf[:, :8] == SENTINEL).all()) and bool((buf[:, 8 + E:] == SENTINEL).all())
        assert intact, f'{name}: written outside its columns'
    assert bool((got['probs_buf'][B * H * L * S:] == SENTINEL).all()), 'probs: written behind its end'
    plain = _apply(dev, dims, q, k, v, d_out, attn_mask, key_pad, p=p, seed=SEED_B)
    tight = _direct(lib, dev, dims, q, k, v, d_out, attn_mask, key_pad, p=p, seed=SEED_B)
    for name in ('out', 'dq', 'dk', 'dv'):
        _same(got[name], plain[name], name)
        _same(tight[name], plain[name], 'tight ' + name)
    _same(got['probs'], tight['probs'], 'probs')
    assert bool((got['probs'] != SENTINEL).all())


# ---- numeric edges ---------------------------------------------------------------------------------------------------

EDGE_SHAPES = [(2, 2, 200, 200, 128), (2, 2, 96, 96, 380)]
_edge_ids = lambda x: 'x'.join(map(str, x)) if isinstance(x, tuple) else str(x)


@pytest.mark.parametrize('dims', EDGE_SHAPES, ids=_edge_ids)
@pytest.mark.parametrize('peak', [12.0, 40.0])
def test_peaked_logits(dev, dims, peak):
    q, k, v, d_out = _inputs(dims, 41)
    q = q * peak
    attn_mask, _ = _masks('future', dims, 41)
    got = _apply(dev, dims, q.to(dev), k.to(dev), v.to(dev), d_out.to(dev), attn_mask, None)
    _check(f'{_edge_ids(dims)} peaked x{peak:g}', dev, dims, q, k, v, d_out, attn_mask, None, got)


@pytest.mark.parametrize('dims', EDGE_SHAPES, ids=_edge_ids)
def test_uniform_logits(dev, lib, dims):
    """q = 0: every score is 0, every stored probability is float32(1) / float32(n) exactly, n the row's allowed keys"""
    B, H, L, S, D = dims
    q, k, v, d_out = _inputs(dims, 42)
    q = torch.zeros_like(q)
    attn_mask, _ = _masks('future', dims, 42)
    got = _direct(lib, dev, dims, q.to(dev), k.to(dev), v.to(dev), d_out.to(dev), attn_mask, None)
    n = (~attn_mask).sum(1).numpy().astype(np.float32)                                  # [L]
    want = np.where(attn_mask.numpy(), np.float32(0), (np.float32(1) / n)[:, None])     # [L, S] float32
    probs = got['probs'].cpu().numpy()
    assert probs.dtype == np.float32 and np.array_equal(probs, np.broadcast_to(want, probs.shape))
    _check(f'{_edge_ids(dims)} uniform', dev, dims, q, k, v, d_out, attn_mask, None, got)


@pytest.mark.parametrize('dims', EDGE_SHAPES, ids=_edge_ids)
def test_shifted_logits(dev, dims):
    """q + u, k + c u with scale c |u|^2 = 300: every score rises by about 300 (softmax does not care; float32 scores do)"""
    B, H, L, S, D = dims
    q, k, v, d_out = _inputs(dims, 43)
    u = torch.full((H * D,), float(D) ** -0.25)      # |u|^2 = sqrt(D) per head
    q, k = q + u, k + 300.0 * u
    attn_mask, _ = _masks('future', dims, 43)
    scores = torch.bmm(R.heads(q.double(), L, B, H, D) * D ** -0.5, R.heads(k.double(), S, B, H, D).transpose(1, 2))
    assert 250.0 < float(scores.mean()) < 350.0
    got = _apply(dev, dims, q.to(dev), k.to(dev), v.to(dev), d_out.to(dev), attn_mask, None)
    _check(f'{_edge_ids(dims)} shifted +300', dev, dims, q, k, v, d_out, attn_mask, None, got)


@pytest.mark.parametrize('dims', EDGE_SHAPES, ids=_edge_ids)
def test_underflowing_exponents(dev, lib, dims):
    """even keys score about +90, odd keys about -90: more than 110 below the row's largest score, where exp underflows
    float32 (2^-149 = exp(-103.3)).  No NaN, the low cluster's probabilities exactly 0, finite gradients in the bound."""
    B, H, L, S, D = dims
    q, k, v, d_out = _inputs(dims, 44)
    w = math.sqrt(90.0 * math.sqrt(D))
    a = torch.full((H * D,), float(D) ** -0.5)        # a unit vector per head
    sign = torch.where(torch.arange(S) % 2 == 0, 1.0, -1.0).repeat_interleave(B)[:, None]       # row s * B + b
    q, k = q + w * a, k + sign * w * a
    attn_mask, _ = _masks('future', dims, 44)
    scores = torch.bmm(R.heads(q.double(), L, B, H, D) * D ** -0.5, R.heads(k.double(), S, B, H, D).transpose(1, 2))
    scores = scores.masked_fill(attn_mask[None], float('-inf'))
    low = (torch.arange(S) % 2 == 1)[None, None, :] & ~attn_mask[None]                            # [1, L, S]
    gap = scores.amax(-1, keepdim=True) - scores
    assert float(gap[low.expand_as(gap)].min()) > 110.0
    got = _direct(lib, dev, dims, q.to(dev), k.to(dev), v.to(dev), d_out.to(dev), attn_mask, None)
    for name in ('probs', 'out', 'dq', 'dk', 'dv'):
        assert bool(torch.isfinite(got[name]).all()), f'{name} is not finite'
    probs = got['probs'].cpu()
    assert bool((probs[low.expand_as(probs)] == 0).all()), 'a probability of the low cluster is not exactly 0'
    assert bool((probs[attn_mask[None].expand_as(probs)] == 0).all())
    _check(f'{_edge_ids(dims)} underflow', dev, dims, q, k, v, d_out, attn_mask, None, got)


@pytest.mark.parametrize('dims', EDGE_SHAPES, ids=_edge_ids)
def test_fully_masked_tracklet_is_nan_forward(dev, lib, dims):
    """every key of tracklet 1 padded: its rows of out and probs are NaN, as torch.softmax gives; tracklet 0 is untouched
    by it.  Forward only."""
    B, H, L, S, D = dims
    q, k, v, d_out = _inputs(dims, 45)
    attn_mask, _ = _masks('future', dims, 45)
    key_pad = torch.zeros(B, S, dtype=torch.bool)
    key_pad[1] = True
    got = _direct(lib, dev, dims, q.to(dev), k.to(dev), v.to(dev), d_out.to(dev), attn_mask, key_pad, backward=False)
    out, probs = got['out'].cpu().view(L, B, H * D), got['probs'].cpu().view(B, H, L, S)
    assert bool(torch.isnan(out[:, 1]).all()) and bool(torch.isnan(probs[1]).all())
    assert bool(torch.isfinite(out[:, 0]).all()) and bool(torch.isfinite(probs[0]).all())
    chain = R.attention(q, k, v, dims, attn_mask, key_pad).view(L, B, H * D)             # what torch.softmax gives
    assert bool(torch.isnan(chain[:, 1]).all())
    _check(f'{_edge_ids(dims)} tracklet 1 masked', dev, dims, q, k, v, d_out, attn_mask, key_pad, {'out': got['out']},
           tracklets=[0])


# ---- dropout ---------------------------------------------------------------------------------------------------------

DROPOUT_CASES = [((2, 2, 200, 200, 384), 0.1, 'future+padding'), ((3, 2, 70, 130, 132), 0.5, 'none'),
                 ((2, 4, 32, 32, 64), 0.1, 'future')]
_drop_ids = lambda x: 'x'.join(map(str, x)) if isinstance(x, tuple) else str(x)


@pytest.mark.parametrize('dims,p,kind', DROPOUT_CASES, ids=_drop_ids)
def test_dropout_mask_is_the_numpy_restatement(dev, dims, p, kind):
    """V = [identity | 0]: the output rows ARE the probabilities after dropout.  The kept elements must be those of
    attn_ref.keep_mask for seeds that differ in the low word, in the high word and in both; the survivors are the
    probabilities times float32(1 / (1 - p)); the dropped share among the allowed elements is p within 5 sigma."""
    B, H, L, S, D = dims
    assert D >= S
    q, k, _, d_out = _inputs(dims, 51)
    attn_mask, key_pad = _masks(kind, dims, 51)
    eye = torch.zeros(S, B, H, D)
    eye[torch.arange(S), :, :, torch.arange(S)] = 1.0                                    # v[s, b, h, :] = e_s
    qd, kd, vd = q.to(dev), k.to(dev), eye.view(S * B, H * D).to(dev)
    rows = lambda t: t.cpu().view(L, B, H, D)[..., :S].permute(1, 2, 0, 3).reshape(B * H, L, S).numpy()
    p0 = rows(_apply(dev, dims, qd, kd, vd, None, attn_mask, key_pad, backward=False)['out'])
    m = R.combined_mask(B, H, L, S, attn_mask, key_pad)
    allowed = np.ones((B * H, L, S), dtype=bool) if m is None else ~m.reshape(B * H, L, S).numpy()
    assert np.array_equal(p0 != 0, allowed)              # unit logits: no allowed probability underflows
    drop_scale = np.float32(1) / (np.float32(1) - np.float32(p))
    masks = []
    for seed in (SEED_A, SEED_B, SEED_C):
        pd = rows(_apply(dev, dims, qd, kd, vd, None, attn_mask, key_pad, p=p, seed=seed, backward=False)['out'])
        keep = R.keep_mask(seed, B * H, L, S, p)
        differ = ((pd != 0) != keep) & allowed
        assert not differ.any(), f'seed {seed}: {int(differ.sum())} of {int(allowed.sum())} elements differ from the hash'
        survivors = np.where(keep, p0 * drop_scale, np.float32(0)).astype(np.float32)
        assert np.array_equal(pd, survivors), f'seed {seed}: a survivor is not its probability times float32(1 / (1 - p))'
        n = int(allowed.sum())
        z = (float(((pd == 0) & allowed).sum()) / n - p) / math.sqrt(p * (1 - p) / n)
        assert abs(z) <= 5.0, f'seed {seed}: dropped share {z:+.2f} sigma from {p}'
        masks.append(pd != 0)
    assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[0], masks[2])


@pytest.mark.parametrize('dims,p,kind', DROPOUT_CASES, ids=_drop_ids)
def test_dropout_forward_and_gradients(dev, dims, p, kind):
    """an ordinary V; the float64 chain and the f32 chain both with the NUMPY mask, not the kernel's.  The first two
    shapes make the key-side workgroups of the backward launch apply the mask at query chunks 64, 128, 192."""
    B, H, L, S, D = dims
    q, k, v, d_out = _inputs(dims, 52)
    attn_mask, key_pad = _masks(kind, dims, 52)
    got = _apply(dev, dims, q.to(dev), k.to(dev), v.to(dev), d_out.to(dev), attn_mask, key_pad, p=p, seed=SEED_B)
    keep = torch.from_numpy(R.keep_mask(SEED_B, B * H, L, S, p))
    _check(f'{_drop_ids(dims)} dropout {p}', dev, dims, q, k, v, d_out, attn_mask, key_pad, got, keep=keep, p=p)


@pytest.mark.parametrize('seed', [SEED_B, SEED_C])
def test_host_seed_is_the_device_seed(dev, lib, seed):
    """seed = value with seed_dev null, in both exports, against seed_dev -> the same value"""
    dims, p = (3, 2, 70, 130, 132), 0.5
    q, k, v, d_out = (t.to(dev) for t in _inputs(dims, 53))
    on_dev = _direct(lib, dev, dims, q, k, v, d_out, None, None, p=p, seed=seed, seed_on_device=True)
    on_host = _direct(lib, dev, dims, q, k, v, d_out, None, None, p=p, seed=seed, seed_on_device=False)
    other = _direct(lib, dev, dims, q, k, v, d_out, None, None, p=p, seed=seed ^ (1 << 40), seed_on_device=False)
    for name in ('probs', 'out', 'dq', 'dk', 'dv'):
        _same(on_host[name], on_dev[name], name)
    assert not torch.equal(other['out'], on_dev['out']) and not torch.equal(other['dq'], on_dev['dq'])


def test_no_dropout_ignores_the_seed(dev):
    dims = RECT_A
    q, k, v, d_out = (t.to(dev) for t in _inputs(dims, 54))
    attn_mask, key_pad = _masks('future+padding', dims, 54)
    plain = _apply(dev, dims, q, k, v, d_out, attn_mask, key_pad, p=0.0, seed=None)
    seeded = _apply(dev, dims, q, k, v, d_out, attn_mask, key_pad, p=0.0, seed=SEED_C)
    for name in ('out', 'dq', 'dk', 'dv'):
        _same(seeded[name], plain[name], name)


def test_two_runs_are_bit_identical(dev, lib):
    """no atomics, fixed summation order: forward and backward twice"""
    dims = RECT_B
    q, k, v, d_out = (t.to(dev) for t in _inputs(dims, 55))
    attn_mask, key_pad = _masks('future+padding', dims, 55)
    one = _direct(lib, dev, dims, q, k, v, d_out, attn_mask, key_pad, p=0.1, seed=SEED_A)
    two = _direct(lib, dev, dims, q, k, v, d_out, attn_mask, key_pad, p=0.1, seed=SEED_A)
    for name in ('out', 'probs', 'dq', 'dk', 'dv'):
        _same(one[name], two[name], name)
    assert bool((one['out'] != SENTINEL).all()) and bool((one['dk'] != SENTINEL).all())


# ---- refusals --------------------------------------------------------------------------------------------------------

REFUSALS = [('L = 257', (1, 2, 257, 32, 32), EUNSUPPORTED), ('S = 257', (1, 2, 32, 257, 32), EUNSUPPORTED),
            ('D = 388', (1, 1, 32, 32, 388), EUNSUPPORTED), ('D = 6', (1, 2, 32, 32, 6), EUNSUPPORTED),
            ('ldq % 4', (1, 2, 32, 32, 32), EINVAL), ('q + 1 float', (1, 2, 32, 32, 32), EINVAL)]


@pytest.mark.parametrize('what,dims,rc', REFUSALS, ids=[r[0].replace(' ', '') for r in REFUSALS])
def test_refusals_touch_nothing(dev, lib, what, dims, rc):
    """every buffer has the full size the arguments claim (a check that failed to refuse could not reach outside them);
    the call returns its error code and the sentinel-filled outputs stay as they were"""
    B, H, L, S, D = dims
    E = H * D
    q, k, v, d_out = (t.to(dev) for t in _inputs(dims, 61))
    if what == 'ldq % 4':
        wide = torch.zeros(L * B, E + 2, device=dev)
        wide[:, :E].copy_(q)
        q = wide[:, :E]
        assert q.stride(0) % 4 == 2
    elif what == 'q + 1 float':
        flat = torch.zeros(L * B * E + 4, device=dev)
        q = flat[1:1 + L * B * E].view(L * B, E)
        assert q.data_ptr() % 16 == 4
    else:
        assert E % 4 == 0
    got = _direct(lib, dev, dims, q, k, v, d_out, None, None, pad=4, spare=16, expect_rc=rc)
    assert got['rc_fwd'] == rc and got['rc_bwd'] == rc
    for name in ('probs_buf', 'out_buf', 'dq_buf', 'dk_buf', 'dv_buf'):
        assert bool((got[name] == SENTINEL).all()), f'{what}: {name} was written'


# ---- the module ------------------------------------------------------------------------------------------------------

def test_module_with_separate_key_takes_the_core(dev, monkeypatch):
    """layers.MultiheadAttention with key is not query, L = 50 and S = 90, a boolean [L, S] mask and a key-padding mask:
    the forward takes the one-launch core (_fused_ok is true), and output, input gradients and parameter gradients are
    those of the same module's operator chain"""
    from objectcentricocccompletion_amd.occ import layers
    torch.manual_seed(0)
    L, S, B, E, H = 50, 90, 3, 256, 4
    g = torch.Generator().manual_seed(71)
    mha = layers.MultiheadAttention(E, H, dropout=0.0).to(dev)
    query, key, value = (torch.randn(n, B, E, generator=g).to(dev) for n in (L, S, S))
    mask = torch.rand(L, S, generator=g) < 0.5
    mask[:, 0] = False
    lens = torch.tensor([S, 1, 40])
    key_pad = (torch.arange(S)[None, :] >= lens[:, None]).to(dev)
    mask = mask.to(dev)
    seen = []
    fused_ok = mha._fused_ok
    monkeypatch.setattr(mha, '_fused_ok', lambda *a: (seen.append(bool(fused_ok(*a))), seen[-1])[1])
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(layers, 'FUSED_ATTENTION', fused)
        mha.zero_grad(set_to_none=True)
        ins = [t.clone().requires_grad_(True) for t in (query, key, value)]
        y, _ = mha(*ins, attn_mask=mask, key_padding_mask=key_pad)
        y.square().sum().backward()
        res[fused] = (y.detach(), [t.grad.clone() for t in ins], [p.grad.clone() for p in mha.parameters()])
    assert seen == [True, False]
    rel = lambda a, e: float((a - e).abs().max() / e.abs().max())
    assert rel(res[True][0], res[False][0]) <= 1e-5
    for a, e in zip(res[True][1] + res[True][2], res[False][1] + res[False][2]):
        assert bool(torch.isfinite(a).all()) and rel(a, e) <= 1e-4
