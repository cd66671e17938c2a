"""The stand-alone LayerNorm(+GELU) kernels (csrc/layernorm_act.hip, csrc/ln_math.hpp, csrc/param_reduce.hpp) against the
float64 reference tests/ln_ref.py, through the C entry points, at the places where the launch code takes another path:
every lane count of the four kernel families (vec, wide, row, generic), the first and last width of each, blocks with
fewer rows than row slots, the row counts at which a block takes a second row per trip and a second trip, and the
numeric edges: the GELU forms far out in both tails, rows with a large offset, constant rows, the folded dropout against
an independent statement of its mask.

Every case checks y, the stored mean / rstd, dx, dgamma and dbeta against per-element bounds derived below (not fitted to
the kernels), the deferred parameter sums bit for bit against the immediate ones, eight canary rows behind every output
and the partial-row count as a literal number.  The backward is handed the float32-rounded statistics of the REFERENCE,
and the reference evaluates the backward from those same numbers: the backward kernels read their statistics, so this is
'the values the kernel read', and the check of the backward does not lean on the forward's rounding.

Each case prints one line 'LNEDGE ...' with the worst error / bound ratio per output (pytest -s shows them).  Measured
on gfx950 when this file was written: float32 outputs use at most a tenth of their bounds (y 0.04, dx 0.09, dgamma /
dbeta 0.10), bf16 outputs 0.995 (the rounding to bf16 itself); max GELU error 6.0e-7 (ln_gelu2), 4.6e-7 (exp form),
derivative 1.9e-7 (ln_gelu_grad2), 1.7e-7 (norm_cdf)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ln_ref as R        # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
EPS = float(np.float32(1e-3))      # the kernels take eps as a float: the reference adds the same number
SENTINEL = -1024.0                 # (a bf16 value)
ON_DEVICE_ABOVE = 2_000_000        # elements: larger cases evaluate the float64 reference on the GPU
THR = round(0.1 * 65536)
SEED = (0x5bd1e995 << 32) | 0x1b873593

# ---- the bounds, stated once -----------------------------------------------------------------------------------------
# u = 2^-24 is the relative error of one float32 operation.
#
# K: the longest chain of dependent float32 operations behind one row quantity.  A lane adds at most 32 channels (the
# generic kernel's VPL = 32; 4 x 8 in the wide kernel, 8 in the row kernel), a row sum then crosses at most 6 shuffle
# steps (64 lanes; the row kernel adds 2 LDS steps instead of nothing), and an element sees at most 6 more operations
# (x - mean, * rstd, * gamma, + beta on the way out; dz * g, - s1, - xhat * s2, * rstd on the way back).  32 + 6 + 6 = 44
# roundings, each at most u of the magnitude it acts on; doubled, as a margin for the terms counted once here that
# occur twice (the variance is a sum of squares of rounded differences): K = 88.
#   y:    |err| <= K u (max_row |z| + rstd |gamma| mean_row |x|) [* 1.13 with the GELU: max |GELU'| = 1.129] + GELU budget
#         The second term is the bound of the mean below carried through z = (x - mean) rstd gamma + beta: an error of
#         the mean reaches z multiplied by rstd gamma, whatever |z| is (a constant row has rstd = eps^-1/2 and z = beta).
#   mean: |err| <= K u sum_row |x| / c
#   rstd: |err| <= rstd (K u + 2^-22): the relative chain bound of the variance (halved by the root, not claimed) plus 2 ulp
#         of rsqrtf
#   dx:   |err| <= K u rstd (|dz gamma| + |s1| + |xhat s2|) + the GELU' budget carried through the same formula
# GELU budget: 2e-6 + 2^-23 |z| for the value and for the derivative (ln_math.hpp: the forms agree to 1e-6; a float32
# emulation with exact reciprocals gives 7.1e-7 at most; the hardware reciprocal is unmeasured, hence 2e-6).  In a
# bound of a row quantity |z| is the row's largest.
# bf16 outputs: one rounding to bf16, 2^-8 |ref|, on top of the float32 bound.  Nothing flat beyond that.
#
# K': additions on the longest path to one dgamma / dbeta.  A block's slab row sums ceil(n / partial rows) input rows
# (trips in registers, then the row slots through LDS: trips + slots <= trips * slots + 1), the reduction adds 1 row
# per running sum (1024 / (32 lanes * 32 sums)), 5 tree steps and 5 butterfly steps: ceil(n / rows) + 1 + 11, doubled.
#   dgamma: |err| <= K' u sum_rows |dz xhat| + sum_rows (GELU' budget |dy xhat|);  dbeta: the same without xhat.
# dy and x are exact inputs in both types, so the same bound holds for bf16 rows.
U = 2.0 ** -24
K = 2 * (32 + 6 + 6)
GELU_ABS, GELU_REL, GELU_LIP = 2e-6, 2.0 ** -23, 1.13
BF16_ULP = 2.0 ** -8


def k_param(n, rows):
    return 2 * (-(-n // rows) + 12)


def _gelu_budget(zabs):
    return GELU_ABS + GELU_REL * zabs


@pytest.fixture(scope='module')
def L():
    from objectcentricocccompletion_amd import _lib
    return _lib


def _within(name, got, ref, tol, ratios):
    """every element of got within tol of ref (NaN fails); records the worst error / bound"""
    err = (got.to(ref.device).double() - ref).abs()
    ok = err <= tol
    if not bool(ok.all()):
        flat = torch.where(ok, torch.zeros_like(err), err / tol.clamp_min(1e-300) + 1).flatten()
        flat = torch.where(torch.isnan(err.flatten()), torch.full_like(flat, float('inf')), flat)
        i = int(flat.argmax())
        raise AssertionError(f'{name}: |got - ref| = {float(err.flatten()[i]):.3e} > bound {float(tol.expand_as(err).flatten()[i]):.3e} '
                             f'at flat index {i} (ref {float(ref.flatten()[i]):.6e}); {int((~ok).sum())} of {ok.numel()} outside')
    ratios[name] = float((err / tol.clamp_min(1e-300)).max())


def _canaries(name, buf, n):
    assert bool((buf[n:].float() == SENTINEL).all()), f'{name}: rows behind row {n} were written'


def _forward(L, dev, xd, gamma, beta, eps, act, drop, with_stats=True):
    n, c = xd.shape
    y = torch.full((n + 8, c), SENTINEL, dtype=xd.dtype, device=dev)
    st = torch.full((n + 8, 2), SENTINEL, dtype=F32, device=dev)
    sp = st.data_ptr() if with_stats else None
    if drop is None:
        rc = L.lib.ococc_layernorm_act_fwd(xd.data_ptr(), n, c, gamma.data_ptr(), beta.data_ptr(), eps, act, y.data_ptr(), sp,
                                           L.dtype_code(xd.dtype), L.stream())
    else:
        rc = L.lib.ococc_layernorm_act_dropout_fwd_bf16(xd.data_ptr(), n, c, gamma.data_ptr(), beta.data_ptr(), eps, act,
                                                        drop[0], drop[1], y.data_ptr(), sp, L.stream())
    assert rc == 0, L.lib.ococc_last_error()
    return y, st


def _backward(L, dev, xd, dyd, gamma, beta, stats, act, drop, immediate):
    """-> dx (with canary rows), dgb [2, c] (NaN where nothing was written), the workspace as floats"""
    n, c = xd.shape
    nbytes = L.lib.ococc_layernorm_act_bwd_workspace_bytes(n, c)
    assert nbytes == 1024 * 2 * c * 4
    ws = torch.full((nbytes // 4,), float('nan'), dtype=F32, device=dev)
    dx = torch.full((n + 8, c), SENTINEL, dtype=xd.dtype, device=dev)
    dgb = torch.full((2, c), float('nan'), dtype=F32, device=dev)
    dg, db = (dgb[0].data_ptr(), dgb[1].data_ptr()) if immediate else (None, None)
    if drop is None:
        rc = L.lib.ococc_layernorm_act_bwd(xd.data_ptr(), dyd.data_ptr(), n, c, gamma.data_ptr(), beta.data_ptr(),
                                           stats.data_ptr(), act, dx.data_ptr(), dg, db, L.dtype_code(xd.dtype),
                                           ws.data_ptr(), nbytes, L.stream())
    else:
        rc = L.lib.ococc_layernorm_act_dropout_bwd_bf16(xd.data_ptr(), dyd.data_ptr(), n, c, gamma.data_ptr(), beta.data_ptr(),
                                                        stats.data_ptr(), act, drop[0], drop[1], dx.data_ptr(), dg, db,
                                                        ws.data_ptr(), nbytes, L.stream())
    assert rc == 0, L.lib.ococc_last_error()
    return dx, dgb, ws


def _reduce(L, ws, rows, c, dgb):
    vp, i32 = ctypes.c_void_p * 1, ctypes.c_int32 * 1
    rc = L.lib.ococc_layernorm_param_reduce_multi(1, vp(ws.data_ptr()), i32(rows), i32(c), vp(dgb[0].data_ptr()),
                                                  vp(dgb[1].data_ptr()), L.stream())
    assert rc == 0, L.lib.ococc_last_error()


def _dropout_scale(thr):
    return float(np.float32(65536.0) / (np.float32(65536.0) - np.float32(thr)))


def _case(L, dev, tag, dtype, c, n, rows, act, x=None, drop=None):
    """One shape through forward, backward and the deferred backward; everything compared with ln_ref.  x: the rows
    (default 2 randn + 0.5); drop = (threshold, seed) takes the dropout entry points.  -> the outputs, for more asserts."""
    rdev = dev if n * c > ON_DEVICE_ABOVE else torch.device('cpu')
    g = torch.Generator(device=rdev).manual_seed(1_000_003 * c + n)   # seeded by shape
    if x is None:
        x = 2 * torch.randn(n, c, generator=g, device=rdev) + 0.5
    x = x.to(rdev).to(dtype)
    gamma = torch.rand(c, generator=g, device=rdev) + 0.5
    beta = 0.1 * torch.randn(c, generator=g, device=rdev)
    noise = torch.randn(n, c, generator=g, device=rdev)
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    keep, scale = None, 1.0
    if drop is not None:
        keep = torch.from_numpy(R.dropout_keep(n, c, drop[0], drop[1])).to(rdev)
        scale = _dropout_scale(drop[0])
    bf16 = dtype == BF16
    ratios = {}

    assert L.lib.ococc_layernorm_act_bwd_partial_rows(n, c, L.dtype_code(dtype)) == rows      # the family this shape is for

    # ---- forward
    y_r, mean_r, rstd_r = R.ln_act(x64, g64, b64, EPS, act, keep, scale)
    xhat = (x64 - mean_r[:, None]) * rstd_r[:, None]
    zabs = (xhat * g64 + b64).abs()
    meanabs = x64.abs().mean(1)
    tol_mean = K * U * meanabs
    tol_rstd = rstd_r * (K * U + 2.0 ** -22)
    tol_y = K * U * (zabs.amax(1, keepdim=True) + (rstd_r * meanabs)[:, None] * g64.abs())
    if act:
        tol_y = GELU_LIP * tol_y + _gelu_budget(zabs)
    tol_y = tol_y * scale
    if bf16:
        tol_y = tol_y + BF16_ULP * y_r.abs()
    xd, gd, bd = x.to(dev).contiguous(), gamma.to(dev), beta.to(dev)
    y, st = _forward(L, dev, xd, gd, bd, EPS, act, drop)
    _within('y', y[:n], y_r, tol_y, ratios)
    _within('mean', st[:n, 0], mean_r, tol_mean, ratios)
    _within('rstd', st[:n, 1], rstd_r, tol_rstd, ratios)
    _canaries('y', y, n)
    _canaries('mean_rstd', st, n)

    # ---- backward, from the reference's statistics as float32
    dy = (noise + 1 + 0.5 * xhat).to(dtype)
    stats = torch.stack([mean_r, rstd_r], 1).float().contiguous()
    t = R.ln_act_backward_terms(x64, dy.double(), g64, b64, EPS, act, keep, scale, stats=(stats[:, 0], stats[:, 1]))
    rstd = t['rstd'][:, None]
    tol_dx = K * U * rstd * (t['dzg'].abs() + t['s1'].abs() + (t['xhat'] * t['s2']).abs())
    kp = k_param(n, rows)
    tol_dg, tol_db = kp * U * t['abs_dgamma'], kp * U * t['abs_dbeta']
    if act:
        budget = _gelu_budget(t['z'].abs().amax(1, keepdim=True))
        a = (t['dy'] * g64).abs()
        ax = t['xhat'].abs()
        tol_dx = tol_dx + rstd * budget * (a + a.mean(1, keepdim=True) + ax * (a * ax).mean(1, keepdim=True))
        tol_dg = tol_dg + (budget * (t['dy'] * t['xhat']).abs()).sum(0)
        tol_db = tol_db + (budget * t['dy'].abs()).sum(0)
    if bf16:
        tol_dx = tol_dx + BF16_ULP * t['dx'].abs()
    dyd, std = dy.to(dev).contiguous(), stats.to(dev)
    dx, dgb, _ = _backward(L, dev, xd, dyd, gd, bd, std, act, drop, immediate=True)
    _within('dx', dx[:n], t['dx'], tol_dx, ratios)
    _within('dgamma', dgb[0], t['dgamma'], tol_dg, ratios)
    _within('dbeta', dgb[1], t['dbeta'], tol_db, ratios)
    _canaries('dx', dx, n)

    # ---- the deferred form: partial rows only, into a workspace of NaN; the sums in the launch that ends a backward pass
    dx2, dgb2, ws2 = _backward(L, dev, xd, dyd, gd, bd, std, act, drop, immediate=False)
    assert bool(torch.isnan(dgb2).all())                                   # (nothing written without the pointers)
    assert bool(torch.isnan(ws2[rows * 2 * c:]).all()), 'partial rows written behind the reported count'
    _reduce(L, ws2, rows, c, dgb2)
    assert torch.equal(dgb2, dgb), 'deferred dgamma / dbeta differ from the immediate ones'
    assert torch.equal(dx2, dx)
    torch.cuda.synchronize()
    print(f'LNEDGE {tag} {"bf16" if bf16 else "f32"} c={c} n={n} act={act} '
          + ' '.join(f'{k}={v:.3f}' for k, v in ratios.items()))
    return dict(y=y[:n], dx=dx[:n], dgb=dgb, keep=keep, y_ref=y_r, terms=t, ratios=ratios)


# ---- the shape table: (family, dtype, c, n, partial rows).  The last column is a literal: it pins the kernel family and
# its grid, and is not computed the way the launch code computes it.
def _table():
    rows = []
    for dt in (F32, BF16):                               # vec, every LPR = c / 8; RPB = 2048 / c row slots per block
        for c in (16, 32, 64, 128, 256, 512):
            rpb = 2048 // c
            rows += [('vec', dt, c, 1, 1), ('vec', dt, c, rpb - 1, 1), ('vec', dt, c, rpb + 1, 2)]
        for n in (4097, 8195, 16385, 32771):             # second row of a trip: backward above 4096, forward above 16384
            rows.append(('vec-trips', dt, 512, n, 1024))
    for n in (131201, 262149, 524419):
        rows.append(('vec-trips', BF16, 16, n, 1024))
    for c in (1024, 1536, 2048):
        rows += [('wide', BF16, c, 1, 1), ('wide', BF16, c, 3, 1), ('wide', BF16, c, 5, 2)]
    for n in (4097, 8195, 32771):
        rows.append(('wide-trips', BF16, 1024, n, 1024))
    for c in (513, 777, 1025, 2047, 2048):
        rows += [('row', F32, c, n, n) for n in (1, 2, 1024)]
    for c in (520, 2047):
        rows += [('row', BF16, c, n, n) for n in (1, 1024)]
    for c in (513, 2047):
        rows.append(('row-to-generic', F32, c, 1025, 257))
    for dt in (F32, BF16):                               # generic: lpr lanes per row, 256 / lpr row slots per block
        for c, lpr in ((1, 1), (3, 1), (4, 1), (5, 2), (8, 2), (9, 4), (24, 8), (40, 16), (100, 32), (131, 64), (264, 64),
                       (511, 64)):
            rows += [('generic', dt, c, 1, 1), ('generic', dt, c, 256 // lpr + 1, 2)]
    for n in (4101, 16389):
        rows.append(('generic-trips', F32, 131, n, 1024))
    for n in (262401, 1048579):
        rows.append(('generic-trips', F32, 3, n, 1024))
    return rows


TABLE = _table()


def _id(case):
    fam, dt, c, n, _ = case
    return f'{fam}-{"bf16" if dt == BF16 else "f32"}-c{c}-n{n}'


@pytest.mark.parametrize('case', TABLE, ids=[_id(c) for c in TABLE])
def test_shape_table(dev, L, case):
    """with the GELU everywhere; the small shapes once more without it (the backward kernels are compiled twice)"""
    fam, dt, c, n, rows = case
    _case(L, dev, fam, dt, c, n, rows, 1)
    if n * c <= ON_DEVICE_ABOVE:
        _case(L, dev, fam, dt, c, n, rows, 0)


def test_shape_table_is_complete():
    """every row of the table this file was written from is present"""
    have = {(f.split('-trips')[0], d, c, n): r for f, d, c, n, r in TABLE}
    assert len(have) == len(TABLE) == 132
    assert have[('vec', BF16, 16, 127)] == 1 and have[('vec', F32, 512, 5)] == 2 and have[('vec', BF16, 16, 524419)] == 1024
    assert have[('wide', BF16, 1536, 5)] == 2 and have[('row', F32, 2047, 1024)] == 1024
    assert have[('row-to-generic', F32, 513, 1025)] == 257 and have[('generic', BF16, 511, 5)] == 2
    assert have[('generic', F32, 3, 1048579)] == 1024 and have[('generic', F32, 100, 9)] == 2


# ---- the GELU forms, with nothing of the LayerNorm arithmetic in between
@pytest.mark.parametrize('family,dtype,c', [('vec', F32, 512), ('row', F32, 2048), ('generic', F32, 510), ('wide', BF16, 2048)],
                         ids=['vec-f32-c512', 'row-f32-c2048', 'generic-f32-c510', 'wide-bf16-c2048'])
def test_gelu_value_and_derivative_in_isolation(dev, L, family, dtype, c):
    """One row of alternating +1 / -1 with eps = 0 and beta = 0: mean = 0 and rstd = 1 exactly, so z = +-gamma[ch] exactly,
    y = GELU(z) and dbeta[ch] = GELU'(z) for dy = 1; gamma runs from 0 to 12.  vec and wide: ln_gelu2 and ln_gelu_grad2;
    row and generic: ln_gelu1 (= ln_gelu2_exp) and norm_cdf / gelu_grad.  (The generic width is 510, not 511: an odd
    number of +-1 has no zero mean; 510 takes the same instance, 64 lanes per row and 8 channels per lane, and
    510 * fl(1 / 510) = 1 in float32 as the exact statistics need.)"""
    x = torch.ones(1, c)
    x[:, 1::2] = -1
    gamma = torch.linspace(0, 12, c)
    beta = torch.zeros(c)
    z = (x[0] * gamma).double()
    xd, gd, bd = x.to(dev).to(dtype), gamma.to(dev), beta.to(dev)
    assert L.lib.ococc_layernorm_act_bwd_partial_rows(1, c, L.dtype_code(dtype)) == 1
    y, st = _forward(L, dev, xd, gd, bd, 0.0, 1, None)
    assert st[0].tolist() == [0.0, 1.0]
    budget = _gelu_budget(z.abs())
    y_r = R.gelu(z)
    err_y = (y[0].cpu().double() - y_r).abs()
    tol_y = budget + (BF16_ULP * y_r.abs() if dtype == BF16 else 0)
    stats = torch.tensor([[0.0, 1.0]], device=dev)
    dx, dgb, _ = _backward(L, dev, xd, torch.ones(1, c, device=dev, dtype=dtype), gd, bd, stats, 1, None, immediate=True)
    d_r = R.gelu_grad(z)
    err_db = (dgb[1].cpu().double() - d_r).abs()
    err_dg = (dgb[0].cpu().double() - d_r * x[0].double()).abs()
    iy, idb = int((err_y / tol_y).argmax()), int((err_db / budget).argmax())
    nz = z != 0
    print(f'LNGELU {family} {"bf16" if dtype == BF16 else "f32"} c={c}: value max |err| {float(err_y.max()):.3e} (z = '
          f'{float(z[int(err_y.argmax())]):.3f}), worst err / bound {float(err_y[iy] / tol_y[iy]):.3f} at z = {float(z[iy]):.3f}, '
          f'max |err| / |z| {float((err_y[nz] / z[nz].abs()).max()):.3e}; derivative max |err| {float(err_db.max()):.3e} (z = '
          f'{float(z[int(err_db.argmax())]):.3f}), worst err / bound {float(err_db[idb] / budget[idb]):.3f}')
    assert bool((err_y <= tol_y).all()), f'GELU value: {float(err_y[iy]):.3e} > {float(tol_y[iy]):.3e} at z = {float(z[iy]):.4f}'
    assert bool((err_db <= budget).all()), f"GELU': {float(err_db[idb]):.3e} > {float(budget[idb]):.3e} at z = {float(z[idb]):.4f}"
    assert bool((err_dg <= budget).all())
    assert bool(torch.isfinite(dx[:1].float()).all())
    _canaries('y', y, 1)
    _canaries('dx', dx, 1)


# ---- rows far from zero
@pytest.mark.parametrize('c', [131, 512, 2048])
def test_offset_rows(dev, L, c):
    """x = 100 + 0.1 randn in float32: the mean is a thousand standard deviations away, a one-pass variance
    (E x^2 - mean^2) has no correct digit left.  The yardstick is what float32 affords on these rows: the distance of
    torch's CPU float32 layer_norm from the float64 reference, times 4."""
    n = 64
    g = torch.Generator().manual_seed(1_000_003 * c + n)
    x = 100 + 0.1 * torch.randn(n, c, generator=g)
    gamma, beta = torch.rand(c, generator=g) + 0.5, 0.1 * torch.randn(c, generator=g)
    y_r, mean_r, rstd_r = R.ln_act(x, gamma, beta, EPS, 0)
    d_torch = float((torch.nn.functional.layer_norm(x, (c,), gamma, beta, EPS).double() - y_r).abs().max())
    y, st = _forward(L, dev, x.to(dev), gamma.to(dev), beta.to(dev), EPS, 0, None)
    d_kernel = float((y[:n].cpu().double() - y_r).abs().max())
    print(f'LNOFFSET c={c}: kernel {d_kernel:.3e}, torch float32 {d_torch:.3e}, bound {4 * d_torch:.3e}')
    assert d_kernel <= 4 * d_torch
    ratios = {}
    _within('mean', st[:n, 0], mean_r, K * U * x.double().abs().mean(1), ratios)
    _within('rstd', st[:n, 1], rstd_r, rstd_r * (K * U + 2.0 ** -22), ratios)
    _canaries('y', y, n)


# ---- constant rows: variance 0, rstd = eps^-1/2, xhat = 0
CONSTANT = [('vec', F32, 512, 5, 2), ('vec', BF16, 512, 5, 2), ('vec', F32, 16, 129, 2), ('wide', BF16, 1024, 5, 2),
            ('row', F32, 777, 3, 3), ('row', BF16, 520, 3, 3), ('generic', F32, 131, 5, 2), ('generic', BF16, 131, 5, 2),
            ('generic', F32, 510, 5, 2)]      # (510: 3 * 510 * fl(1 / 510) is not 3 in float32, the mean is one ulp off)


@pytest.mark.parametrize('family,dtype,c,n,rows', CONSTANT, ids=[_id(c) for c in CONSTANT])
@pytest.mark.parametrize('act', [1, 0])
def test_constant_rows(dev, L, family, dtype, c, n, rows, act):
    out = _case(L, dev, 'constant-' + family, dtype, c, n, rows, act, x=torch.full((n, c), 3.0))
    t = out['terms']
    assert float(t['xhat'].abs().max()) == 0.0 and float((t['rstd'] - EPS ** -0.5).abs().max()) < 1e-5
    beta = t['z'][0]                                          # z = beta where xhat = 0
    assert torch.equal(out['y_ref'], (R.gelu(beta) if act else beta).expand(n, c))     # what _case compared y with
    assert bool(torch.isfinite(out['dx'].float()).all()) and bool(torch.isfinite(out['dgb']).all())


# ---- the folded dropout against ln_ref.dropout_keep
@pytest.mark.parametrize('c,rows', [(16, 3), (512, 75), (1024, 75), (2048, 75)])
def test_dropout_against_the_independent_mask(dev, L, c, rows):
    n = 300
    out = _case(L, dev, 'dropout', BF16, c, n, rows, 1, drop=(THR, SEED))
    keep = out['keep'].to(dev)
    y = out['y'].float()
    assert 0.05 < 1.0 - float(keep.float().mean()) < 0.15
    assert float(y[~keep].abs().max()) == 0.0                              # exactly zero where dropped
    # the high half of the seed reaches the mask, in the kernel as in the reference
    g = torch.Generator().manual_seed(1_000_003 * c + n)            # (the inputs of _case)
    x = (2 * torch.randn(n, c, generator=g) + 0.5).bfloat16()
    gamma, beta = torch.rand(c, generator=g) + 0.5, 0.1 * torch.randn(c, generator=g)
    x, gamma, beta = x.to(dev), gamma.to(dev), beta.to(dev)
    y1, _ = _forward(L, dev, x, gamma, beta, EPS, 1, (THR, SEED))
    assert torch.equal(y1[:n], out['y'])
    y2, _ = _forward(L, dev, x, gamma, beta, EPS, 1, (THR, SEED + 2 ** 32))
    keep2 = torch.from_numpy(R.dropout_keep(n, c, THR, SEED + 2 ** 32)).to(dev)
    assert not torch.equal(keep2, keep)
    y2 = y2[:n].float()
    assert float(y2[~keep2].abs().max()) == 0.0           # (the kept values: the case below, in full)
    _case(L, dev, 'dropout', BF16, c, n, rows, 0, drop=(THR, SEED + 2 ** 32))


# ---- what returns before any launch
def test_contracts_in_front_of_the_launch(dev, L):
    lib = L.lib
    n, c = 5, 131
    x = torch.randn(n, c, device=dev)
    gamma, beta = torch.ones(c, device=dev), torch.zeros(c, device=dev)
    st = torch.zeros(n, 2, device=dev)
    nan = float('nan')
    dx = torch.full((n, c), SENTINEL, device=dev)
    ws = torch.empty(1024 * 2 * 2049, device=dev)
    for dt in (F32, BF16):
        # no rows: the sums are zero
        dgb = torch.full((2, c), nan, device=dev)
        assert lib.ococc_layernorm_act_bwd(None, None, 0, c, gamma.data_ptr(), beta.data_ptr(), None, 1, None, dgb[0].data_ptr(),
                                           dgb[1].data_ptr(), L.dtype_code(dt), None, 0, L.stream()) == 0
        assert float(dgb.abs().max()) == 0.0
        assert lib.ococc_layernorm_act_fwd(None, 0, c, gamma.data_ptr(), beta.data_ptr(), EPS, 1, None, None, L.dtype_code(dt),
                                           L.stream()) == 0
        assert lib.ococc_layernorm_act_bwd_partial_rows(0, c, L.dtype_code(dt)) == 0
    dgb = torch.full((2, c), nan, device=dev)
    assert lib.ococc_layernorm_act_dropout_bwd_bf16(None, None, 0, c, gamma.data_ptr(), beta.data_ptr(), None, 1, THR, SEED, None,
                                                    dgb[0].data_ptr(), dgb[1].data_ptr(), None, 0, L.stream()) == 0
    assert float(dgb.abs().max()) == 0.0
    # more than 2048 channels: unsupported, in both directions
    wide = torch.randn(n, 2049, device=dev)
    gw, bw = torch.ones(2049, device=dev), torch.zeros(2049, device=dev)
    out = torch.full((n, 2049), SENTINEL, device=dev)
    assert lib.ococc_layernorm_act_bwd_workspace_bytes(n, 2049) == ws.numel() * 4
    assert lib.ococc_layernorm_act_fwd(wide.data_ptr(), n, 2049, gw.data_ptr(), bw.data_ptr(), EPS, 1, out.data_ptr(), st.data_ptr(),
                                       L.F32, L.stream()) == -3
    assert lib.ococc_layernorm_act_bwd(wide.data_ptr(), wide.data_ptr(), n, 2049, gw.data_ptr(), bw.data_ptr(), st.data_ptr(), 1,
                                       out.data_ptr(), gw.data_ptr(), bw.data_ptr(), L.F32, ws.data_ptr(), ws.numel() * 4,
                                       L.stream()) == -3
    assert bool((out == SENTINEL).all())
    # a workspace one byte short
    need = lib.ococc_layernorm_act_bwd_workspace_bytes(n, c)
    dgb = torch.full((2, c), nan, device=dev)
    args = (x.data_ptr(), x.data_ptr(), n, c, gamma.data_ptr(), beta.data_ptr(), st.data_ptr(), 1, dx.data_ptr(), dgb[0].data_ptr(),
            dgb[1].data_ptr(), L.F32, ws.data_ptr())
    assert lib.ococc_layernorm_act_bwd(*args, need - 1, L.stream()) == -1
    assert bool((dx == SENTINEL).all()) and bool(torch.isnan(dgb).all())
    # the dropout entry points: widths without a dropout kernel, a threshold that would drop everything
    xb = torch.randn(n, 777, device=dev).bfloat16()
    g7, b7 = torch.ones(777, device=dev), torch.zeros(777, device=dev)
    yb = torch.full((n, 777), SENTINEL, device=dev, dtype=BF16)
    assert lib.ococc_layernorm_act_dropout_fwd_bf16(xb.data_ptr(), n, 777, g7.data_ptr(), b7.data_ptr(), EPS, 1, THR, SEED,
                                                    yb.data_ptr(), st.data_ptr(), L.stream()) == -3
    assert lib.ococc_layernorm_act_dropout_bwd_bf16(xb.data_ptr(), xb.data_ptr(), n, 777, g7.data_ptr(), b7.data_ptr(), st.data_ptr(),
                                                    1, THR, SEED, yb.data_ptr(), g7.data_ptr(), b7.data_ptr(), ws.data_ptr(),
                                                    ws.numel() * 4, L.stream()) == -3
    x5 = torch.randn(n, 512, device=dev).bfloat16()
    g5, b5 = torch.ones(512, device=dev), torch.zeros(512, device=dev)
    y5 = torch.full((n, 512), SENTINEL, device=dev, dtype=BF16)
    assert lib.ococc_layernorm_act_dropout_fwd_bf16(x5.data_ptr(), n, 512, g5.data_ptr(), b5.data_ptr(), EPS, 1, 65536, SEED,
                                                    y5.data_ptr(), st.data_ptr(), L.stream()) == -1
    assert lib.ococc_layernorm_act_dropout_bwd_bf16(x5.data_ptr(), x5.data_ptr(), n, 512, g5.data_ptr(), b5.data_ptr(), st.data_ptr(),
                                                    1, 65536, SEED, y5.data_ptr(), g5.data_ptr(), b5.data_ptr(), ws.data_ptr(),
                                                    ws.numel() * 4, L.stream()) == -1
    torch.cuda.synchronize()
    assert bool((yb == SENTINEL).all()) and bool((y5 == SENTINEL).all())
    assert float(g7.min()) == 1.0 and float(g5.min()) == 1.0 and float(gw.min()) == 1.0      # (no sums written either)


@pytest.mark.parametrize('dtype,c,n', [(F32, 512, 9), (BF16, 64, 40), (BF16, 1024, 5), (F32, 777, 3), (F32, 131, 9), (BF16, 9, 70)],
                         ids=['vec-f32', 'vec-bf16', 'wide-bf16', 'row-f32', 'generic-f32', 'generic-bf16'])
def test_forward_without_statistics(dev, L, dtype, c, n):
    """mean_rstd = NULL (inference): the same y bits"""
    g = torch.Generator().manual_seed(c)
    x = (2 * torch.randn(n, c, generator=g) + 0.5).to(dtype).to(dev)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(dev), (0.1 * torch.randn(c, generator=g)).to(dev)
    y1, st1 = _forward(L, dev, x, gamma, beta, EPS, 1, None)
    y0, st0 = _forward(L, dev, x, gamma, beta, EPS, 1, None, with_stats=False)
    assert torch.equal(y0, y1) and bool((st0 == SENTINEL).all()) and not bool((st1[:n] == SENTINEL).any())
