"""GPU parity, sparse-conv side (B3, B4, B5): rulebook bit-exact vs the oracle, conv
forward/backward vs the oracle on the same bf16-rounded operands, module level autograd,
and size-independent properties at the benchmark shape (64 x 40^3)."""
import collections
import contextlib

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _voxels(rng, B, shape, density, shuffle):
    mask = rng.random((B,) + tuple(shape)) < density
    idx = np.argwhere(mask).astype(np.int32)
    if shuffle:
        idx = idx[rng.permutation(len(idx))]
    return idx


@pytest.mark.parametrize('case', [
    dict(B=1, shape=(4, 4, 4), density=0.5, shuffle=False, ks=(3, 3, 3)),
    dict(B=3, shape=(9, 10, 11), density=0.2, shuffle=True, ks=(3, 3, 3)),
    dict(B=2, shape=(40, 40, 40), density=0.03, shuffle=False, ks=(3, 3, 3)),
    dict(B=2, shape=(12, 12, 12), density=0.9, shuffle=True, ks=(3, 3, 3)),
    dict(B=2, shape=(1, 20, 20), density=0.3, shuffle=True, ks=(1, 3, 3)),
    dict(B=1, shape=(6, 6, 6), density=0.4, shuffle=True, ks=(3, 1, 3)),
])
def test_subm_rulebook_bit_exact(dev, case):
    from objectcentricocccompletion_amd.spconv import ops
    rng = np.random.default_rng(11)
    idx = _voxels(rng, case['B'], case['shape'], case['density'], case['shuffle'])
    outids, pairs, num = ops.get_indice_pairs(torch.from_numpy(idx).to(dev), case['B'], list(case['shape']),
                                              list(case['ks']), 1, 0, 1, 0, subm=True)
    ep, en = O.subm_rulebook(idx, case['B'], case['shape'], case['ks'])
    assert np.array_equal(num.cpu().numpy(), en)
    assert np.array_equal(pairs.cpu().numpy(), ep)       # same order as the CPU functor, -1 fill included
    assert torch.equal(outids.cpu(), torch.from_numpy(idx))
    # the gather table agrees with the pairs: table[k][out] = in
    table, mask, rows = pairs._ococc.tables[(False, 'fwd')]
    t = table.cpu().numpy()
    for k in range(len(en)):
        exp = np.full(len(idx), -1, np.int32)
        exp[ep[k, 1, :en[k]]] = ep[k, 0, :en[k]]
        assert np.array_equal(t[k], exp)
    if mask is not None:
        m = mask.cpu().numpy().view(np.uint32)
        for b in range(len(m)):
            exp = 0
            for k in range(len(en)):
                if (t[k, b * 16:(b + 1) * 16] >= 0).any():
                    exp |= 1 << k
            assert int(m[b]) == exp


def test_rulebook_empty_and_single(dev):
    from objectcentricocccompletion_amd.spconv import ops
    o, p, n = ops.get_indice_pairs(torch.zeros((0, 4), dtype=torch.int32, device=dev), 1, [8, 8, 8], 3, subm=True)
    assert p.shape == (27, 2, 0) and int(n.sum()) == 0
    o, p, n = ops.get_indice_pairs(torch.tensor([[0, 7, 7, 7]], dtype=torch.int32, device=dev), 1, [8, 8, 8], 3, subm=True)
    assert n.tolist() == [0] * 13 + [1] + [0] * 13 and p[13, :, 0].tolist() == [0, 0]


def _conv_case(rng, dev, B, shape, density, cin, cout, shuffle=True):
    from objectcentricocccompletion_amd.spconv import ops
    idx = _voxels(rng, B, shape, density, shuffle)
    n = len(idx)
    x = O.bf16_round(rng.standard_normal((n, cin)).astype(np.float32))
    w = O.bf16_round(rng.standard_normal((3, 3, 3, cin, cout)).astype(np.float32) * 0.2)
    dy = O.bf16_round(rng.standard_normal((n, cout)).astype(np.float32))
    _, pairs, num = ops.get_indice_pairs(torch.from_numpy(idx).to(dev), B, list(shape), 3, subm=True)
    ep, en = O.subm_rulebook(idx, B, shape)
    return idx, x, w, dy, pairs, num, ep, en


# fp32 accumulation of exact bf16 products: only summation order differs from the oracle
TOL = dict(rtol=1e-4, atol=2e-4)


@contextlib.contextmanager
def _kernel_family(ops, family):
    """pin the convolution kernel family for one test (None: what an unmeasured density selects -- the voxel-order
    output-stationary kernels; 'sorted': rows in neighbour-pattern order, the kernel bench.py's configs[1] step runs;
    'tile': the compact-then-multiply tile kernel) and hand back the launch counter to assert on"""
    keep = ops.SORTED_CONV, ops.SPARSE_TILE_CONV
    ops.SORTED_CONV = True if family == 'sorted' else keep[0]
    ops.SPARSE_TILE_CONV = {'sorted': False, 'tile': True}.get(family, keep[1])
    before = collections.Counter(ops.launches)
    ran = collections.Counter()
    try:
        yield ran
    finally:
        ops.SORTED_CONV, ops.SPARSE_TILE_CONV = keep
        ran.update(ops.launches - before)


# channel pairs the neighbour-pattern-order kernel is instantiated for (csrc/sparse_conv_sorted.hip)
_SORTED_SHAPES = {(32, 32), (32, 64), (64, 32), (64, 64), (64, 128), (128, 64), (32, 128), (128, 32)}


@pytest.mark.parametrize('family', [None, 'sorted'])
@pytest.mark.parametrize('cin,cout', [(16, 32), (32, 64), (64, 128), (128, 64), (64, 32), (128, 128), (16, 16), (5, 7), (48, 96)])
@pytest.mark.parametrize('density', [0.04, 0.6])
def test_subm_conv_forward_backward_vs_oracle(dev, cin, cout, density, family):
    """every kernel family against the oracle DIRECTLY (the pattern-order kernel was only compared
    with the voxel-order kernel)"""
    from objectcentricocccompletion_amd.spconv import ops
    if family == 'sorted' and (cin, cout) not in _SORTED_SHAPES:
        pytest.skip('no pattern-order instantiation for this channel pair: the default case covers it')
    with _kernel_family(ops, family) as ran:
        _subm_conv_vs_oracle(ops, dev, cin, cout, density)
    if family == 'sorted':
        assert ran['sorted'] >= 3 and ran['stationary'] == 0 and ran['tile'] == 0, dict(ran)   # f32 fwd, bf16 fwd, dgrad
    else:
        assert ran['sorted'] == 0, dict(ran)


def _subm_conv_vs_oracle(ops, dev, cin, cout, density):
    rng = np.random.default_rng(cin * 1000 + cout)
    idx, x, w, dy, pairs, num, ep, en = _conv_case(rng, dev, 2, (14, 15, 16), density, cin, cout)
    n = len(idx)
    xt, wt, dyt = (torch.from_numpy(a).to(dev) for a in (x, w, dy))
    y = ops.indice_conv(xt, wt, pairs, num, n, False, True)            # f32 in -> f32 out
    ey = O.indice_conv(x, w, ep, en, n, subm=True)
    assert y.dtype == torch.float32 and np.allclose(y.cpu().numpy(), ey, **TOL)
    yb = ops.indice_conv(xt.bfloat16(), wt.bfloat16(), pairs, num, n, False, True)  # bf16 out
    assert yb.dtype == torch.bfloat16
    assert torch.equal(yb, y.bfloat16())    # bf16 output == RNE rounding of the f32 accumulators
    din, dw = ops.indice_conv_backward(xt, wt, dyt, pairs, num, False, True)
    edin, edw = O.indice_conv_backward(x, w, dy, ep, en, subm=True)
    assert np.allclose(din.cpu().numpy(), edin, **TOL)
    scale = max(1.0, float(np.abs(edw).max()))
    assert np.allclose(dw.cpu().numpy(), edw, rtol=1e-4, atol=2e-4 * scale)


def test_user_supplied_rulebook_without_cached_tables(dev):
    """indice_conv called the reference way with bare pair tensors (e.g. produced elsewhere)."""
    from objectcentricocccompletion_amd.spconv import ops
    rng = np.random.default_rng(5)
    idx, x, w, dy, pairs, num, ep, en = _conv_case(rng, dev, 1, (10, 10, 10), 0.3, 32, 32)
    bare_pairs = torch.from_numpy(ep).to(dev)
    bare_num = torch.from_numpy(en).to(dev)
    xt, wt, dyt = (torch.from_numpy(a).to(dev) for a in (x, w, dy))
    y = ops.indice_conv(xt, wt, bare_pairs, bare_num, len(idx), False, True)
    assert np.allclose(y.cpu().numpy(), O.indice_conv(x, w, ep, en, len(idx), subm=True), **TOL)
    din, dw = ops.indice_conv_backward(xt, wt, dyt, bare_pairs, bare_num, False, True)
    edin, edw = O.indice_conv_backward(x, w, dy, ep, en, subm=True)
    assert np.allclose(din.cpu().numpy(), edin, **TOL) and np.allclose(dw.cpu().numpy(), edw, rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('c', [16, 32, 128, 131, 777, 1024, 1536, 2048])   # (f32 rows wider than 512 channels: one row per workgroup)
@pytest.mark.parametrize('act', ['none', 'gelu'])
def test_layernorm_act_vs_torch(dev, dtype, c, act):
    from objectcentricocccompletion_amd.norm import layer_norm_act
    g = torch.Generator().manual_seed(c)
    n = 1000 if c < 1000 else 67
    x = (torch.randn(n, c, generator=g) * 2 + 0.5).to(dtype)
    w = torch.rand(c, generator=g) + 0.5
    b = torch.randn(c, generator=g) * 0.1
    dy = torch.randn(n, c, generator=g).to(dtype)
    xd = x.to(dev).requires_grad_(True)
    wd, bd = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    y = layer_norm_act(xd, wd, bd, 1e-3, act)
    y.backward(dy.to(dev))
    xr = x.double().requires_grad_(True)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (c,), wr, br, 1e-3)
    if act == 'gelu':
        yr = torch.nn.functional.gelu(yr)
    yr.backward(dy.double())
    if dtype == torch.float32:
        tol = dict(rtol=1e-4, atol=1e-5)
    else:  # output rounded to bf16 once: half an ulp = 2^-9 relative
        tol = dict(rtol=2 ** -8, atol=2 ** -8)
    assert torch.allclose(y.detach().cpu().double(), yr.detach(), **tol)
    assert torch.allclose(xd.grad.cpu().double(), xr.grad, rtol=tol['rtol'], atol=tol['atol'] * 4)
    assert torch.allclose(wd.grad.cpu().double(), wr.grad, rtol=1e-3, atol=1e-3 * float(wr.grad.abs().max()))
    assert torch.allclose(bd.grad.cpu().double(), br.grad, rtol=1e-3, atol=1e-3 * float(br.grad.abs().max()))


@pytest.mark.parametrize('n,c', [(1, 1024), (1024, 1024), (1025, 2048), (3000, 1536)])
def test_layernorm_of_few_wide_f32_rows(dev, n, c):
    """f32 rows wider than 512 channels: one row per workgroup up to 1024 rows (the backward's workspace holds 1024 partial
    rows), the generic kernel beyond -- both against torch in float64, and the partial-row count the library reports."""
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.norm import layer_norm_act
    assert L.lib.ococc_layernorm_act_bwd_partial_rows(n, c, L.dtype_code(torch.float32)) == (n if n <= 1024 else min(-(-n // 4), 1024))
    g = torch.Generator().manual_seed(n + c)
    x = torch.randn(n, c, generator=g) * 2 + 0.5
    w, b = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1
    dy = torch.randn(n, c, generator=g)
    xd, wd, bd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    y = layer_norm_act(xd, wd, bd, 1e-3, 'gelu')
    y.backward(dy.to(dev))
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = torch.nn.functional.gelu(torch.nn.functional.layer_norm(xr, (c,), wr, br, 1e-3))
    yr.backward(dy.double())
    assert torch.allclose(y.detach().cpu().double(), yr.detach(), rtol=1e-4, atol=1e-5)
    assert torch.allclose(xd.grad.cpu().double(), xr.grad, rtol=1e-4, atol=4e-5)
    assert torch.allclose(wd.grad.cpu().double(), wr.grad, rtol=1e-3, atol=1e-3 * float(wr.grad.abs().max()))
    assert torch.allclose(bd.grad.cpu().double(), br.grad, rtol=1e-3, atol=1e-3 * float(br.grad.abs().max()))


def test_sparse_convmodule_autograd_vs_reference_math(dev):
    """conv -> LN(eps 1e-3) -> GELU stack of make_sparse_convmodule, bf16 features, compared
    with the same network evaluated in float64 from the oracle's rulebook."""
    from objectcentricocccompletion_amd.sparse_block import make_sparse_convmodule
    from objectcentricocccompletion_amd.spconv import SparseConvTensor
    rng = np.random.default_rng(21)
    B, shape = 4, (16, 16, 16)
    idx = _voxels(rng, B, shape, 0.15, False)
    n = len(idx)
    torch.manual_seed(0)
    chans = [16, 32, 64]
    layers = [make_sparse_convmodule(chans[i], chans[i + 1], 3, 'subm1', padding=1, conv_type='SubMConv3d',
                                     act_type='gelu', norm_cfg=dict(type='LN', eps=1e-3)).to(dev)
              for i in range(2)]
    x = O.bf16_round(rng.standard_normal((n, 16)).astype(np.float32))
    xt = torch.from_numpy(x).to(dev).bfloat16()
    st = SparseConvTensor(xt, torch.from_numpy(idx).to(dev), list(shape), B)
    for m in layers:
        st = m(st)
    out = st.features
    assert out.dtype == torch.bfloat16 and 'subm1' in st.indice_dict
    loss = (out.float() ** 2).sum()
    loss.backward()
    # float64 reference from the oracle rulebook
    ep, en = O.subm_rulebook(idx, B, shape)
    h = torch.from_numpy(x).double()
    params = []
    for m in layers:
        w = m[0].weight.detach().cpu().double().requires_grad_(True)
        g = m[1].weight.detach().cpu().double().requires_grad_(True)
        b = m[1].bias.detach().cpu().double().requires_grad_(True)
        params.append((w, g, b))
        wb = w.detach().bfloat16().double() + (w - w.detach())   # the kernel sees bf16-rounded weights
        y = torch.zeros(n, w.shape[-1], dtype=torch.float64)
        w27 = wb.reshape(27, w.shape[-2], w.shape[-1])
        for k in range(27):
            if en[k]:
                y = y.index_add(0, torch.from_numpy(ep[k, 1, :en[k]]).long(),
                                h[torch.from_numpy(ep[k, 0, :en[k]]).long()] @ w27[k])
        h = torch.nn.functional.gelu(torch.nn.functional.layer_norm(y, (y.shape[1],), g, b, 1e-3))
    (h ** 2).sum().backward()
    rel = lambda a, b_: float((a.detach().double().cpu() - b_).abs().max() / (b_.abs().max() + 1e-12))
    assert rel(out, h.detach()) < 2e-2          # two bf16 layers deep
    for m, (w, g, b) in zip(layers, params):
        assert rel(m[0].weight.grad, w.grad) < 5e-2
        assert rel(m[1].weight.grad, g.grad) < 5e-2
        assert rel(m[1].bias.grad, b.grad) < 5e-2


def test_conv_properties_at_benchmark_scale(dev):
    """64 grids x 40^3 with ~2000 active voxels each (the bench shape), where the oracle
    would take minutes: linearity, determinism, rulebook symmetry, adjoint identity."""
    from objectcentricocccompletion_amd.spconv import ops
    g = torch.Generator().manual_seed(3)
    B = 64
    cells = torch.stack([torch.randperm(64000, generator=g)[:2000].sort().values + b * 64000 for b in range(B)]).flatten()
    idx = torch.stack([cells // 64000, (cells // 1600) % 40, (cells // 40) % 40, cells % 40], 1).int().to(dev)
    n = idx.shape[0]
    _, pairs, num = ops.get_indice_pairs(idx, B, [40, 40, 40], 3, subm=True)
    numc = num.cpu()
    assert int(numc[13]) == n
    assert torch.equal(numc, numc.flip(0))                       # offset k <-> 26-k symmetry
    p = pairs.cpu()
    for k in (0, 5, 12):
        a = p[k, :, :numc[k]]
        b = p[26 - k, :, :numc[k]]
        sa = a[:, torch.argsort(a[0] * n + a[1])]
        sb = b.flip(0)
        sb = sb[:, torch.argsort(sb[0] * n + sb[1])]
        assert torch.equal(sa, sb)
    cin, cout = 64, 128
    x1 = torch.randn(n, cin, generator=g).to(dev).bfloat16()
    x2 = torch.randn(n, cin, generator=g).to(dev).bfloat16()
    w = (torch.randn(3, 3, 3, cin, cout, generator=g) * 0.05).to(dev).bfloat16()
    y1 = ops.indice_conv(x1.float(), w, pairs, num, n, False, True)
    y1b = ops.indice_conv(x1.float(), w, pairs, num, n, False, True)
    assert torch.equal(y1, y1b)                                   # deterministic, run to run
    y2 = ops.indice_conv(x2.float(), w, pairs, num, n, False, True)
    xs = (x1.float() + x2.float())                                # rounded to bf16 inside the op
    ys = ops.indice_conv(xs, w, pairs, num, n, False, True)
    # linearity up to that one bf16 rounding of the summed input
    assert float((ys - (y1 + y2)).abs().mean()) < 2e-2 * float(ys.abs().mean())
    # adjoint identity <conv(x), dy> == <x, dgrad(dy)> ties forward and dgrad together
    dy = torch.randn(n, cout, generator=g).to(dev).bfloat16().float()
    din, dw = ops.indice_conv_backward(x1.float(), w, dy, pairs, num, False, True)
    lhs = float((y1.double() * dy.double()).sum())
    rhs = float((x1.double() * din.double()).sum())
    assert abs(lhs - rhs) < 1e-3 * max(abs(lhs), 1.0)
    # <dW, W> == <conv(x), dy>
    rhs2 = float((dw.double() * w.double()).sum())
    assert abs(lhs - rhs2) < 1e-3 * max(abs(lhs), 1.0)


def _match_sorted(outids_oracle):
    """permutation: oracle output row (first-appearance order) -> row in sorted order."""
    o = outids_oracle.astype(np.int64)
    key = ((o[:, 0] * 10000 + o[:, 1]) * 10000 + o[:, 2]) * 10000 + o[:, 3]
    order = np.argsort(key, kind='stable')
    perm = np.empty(len(o), np.int64)
    perm[order] = np.arange(len(o))
    return order, perm


@pytest.mark.parametrize('case', [
    dict(ks=(3, 3, 3), stride=(2, 2, 2), pad=(1, 1, 1), transpose=False),
    dict(ks=(3, 3, 3), stride=(1, 1, 1), pad=(0, 0, 0), transpose=False),
    dict(ks=(3, 1, 1), stride=(2, 1, 1), pad=(0, 0, 0), transpose=False),
    dict(ks=(2, 2, 2), stride=(2, 2, 2), pad=(0, 0, 0), transpose=False),
    dict(ks=(3, 3, 3), stride=(2, 2, 2), pad=(1, 1, 1), transpose=True),
])
def test_regular_and_transposed_rulebook_vs_oracle(dev, case):
    """SparseConv3d / transposed rulebooks: same active outputs, same pairs per offset in the same
    (ascending input) order; output rows are numbered sorted instead of by first appearance."""
    from objectcentricocccompletion_amd.spconv import ops
    rng = np.random.default_rng(17)
    B, shape = 3, (9, 10, 11)
    idx = _voxels(rng, B, shape, 0.15, True)
    ks, st, pd = case['ks'], case['stride'], case['pad']
    if case['transpose']:
        oshape = ops.get_deconv_output_size(list(shape), list(ks), list(st), list(pd), [1, 1, 1], [0, 0, 0])
    else:
        oshape = ops.get_conv_output_size(list(shape), list(ks), list(st), list(pd), [1, 1, 1])
    eo, ep, en = O.conv_rulebook(idx, B, oshape, ks, st, pd, (1, 1, 1), transpose=case['transpose'])
    outids, pairs, num = ops.get_indice_pairs(torch.from_numpy(idx).to(dev), B, list(shape), list(ks), list(st),
                                              list(pd), 1, 0, subm=False, transpose=case['transpose'])
    order, perm = _match_sorted(eo)
    assert np.array_equal(outids.cpu().numpy(), eo[order])
    assert np.array_equal(num.cpu().numpy(), en)
    p = pairs.cpu().numpy()
    for k in range(len(en)):
        assert np.array_equal(p[k, 0, :en[k]], ep[k, 0, :en[k]])
        assert np.array_equal(p[k, 1, :en[k]], perm[ep[k, 1, :en[k]]])
        assert (p[k, :, en[k]:] == -1).all()


def test_sparse_conv3d_and_inverse_modules_vs_dense(dev):
    """SparseConv3d (stride 2) followed by its SparseInverseConv3d partner, forward and backward,
    against dense conv3d / the oracle's inverse formulation."""
    from objectcentricocccompletion_amd.spconv import SparseConv3d, SparseConvTensor, SparseInverseConv3d
    rng = np.random.default_rng(23)
    B, shape, cin, cmid = 2, (8, 10, 12), 16, 32
    idx = _voxels(rng, B, shape, 0.2, True)
    n = len(idx)
    torch.manual_seed(1)
    down = SparseConv3d(cin, cmid, 3, stride=2, padding=1, bias=False, indice_key='d1').to(dev)
    up = SparseInverseConv3d(cmid, cin, 3, indice_key='d1', bias=False).to(dev)
    x = O.bf16_round(rng.standard_normal((n, cin)).astype(np.float32))
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    st = SparseConvTensor(xt, torch.from_numpy(idx).to(dev), list(shape), B)
    mid = down(st)
    out = up(mid)
    assert out.features.shape == (n, cin) and torch.equal(out.indices.cpu(), torch.from_numpy(idx))
    (out.features ** 2).sum().backward()
    # reference math from the oracle rulebook (first-appearance numbering) in float64
    oshape = [(s + 2 - 3) // 2 + 1 for s in shape]
    eo, ep, en = O.conv_rulebook(idx, B, oshape, (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1))
    order, perm = _match_sorted(eo)
    w1 = O.bf16_round(down.weight.detach().cpu().numpy())
    w2 = O.bf16_round(up.weight.detach().cpu().numpy())
    ymid = O.indice_conv(x, w1, ep, en, len(eo))
    assert np.allclose(mid.features.detach().cpu().numpy(), ymid[order], rtol=1e-3, atol=2e-3)
    yout = O.indice_conv(O.bf16_round(ymid), w2, ep, en, n, inverse=True)
    assert np.allclose(out.features.detach().cpu().numpy(), yout, rtol=2e-2, atol=3e-2)  # bf16 hop in between
    # dense cross-check of the strided conv
    dense = torch.zeros((B,) + shape + (cin,))
    dense[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = torch.from_numpy(x)
    yd = torch.nn.functional.conv3d(dense.permute(0, 4, 1, 2, 3), torch.from_numpy(w1).permute(4, 3, 0, 1, 2),
                                    padding=1, stride=2).permute(0, 2, 3, 4, 1)
    oi = mid.indices.cpu().numpy()
    assert np.allclose(mid.features.detach().cpu().numpy(), yd[oi[:, 0], oi[:, 1], oi[:, 2], oi[:, 3]].numpy(),
                       rtol=1e-3, atol=2e-3)
    # gradients: adjoint identity through both layers
    g = xt.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
    assert down.weight.grad is not None and up.weight.grad is not None
    din, dw2 = O.indice_conv_backward(O.bf16_round(ymid), w2, O.bf16_round(2 * yout), ep, en, inverse=True)
    assert rel_close(up.weight.grad.cpu().numpy(), dw2, 5e-2)


def rel_close(a, b, tol):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12)) < tol


def test_subm_rulebook_sorted_grid_fast_path_matches_generic(dev):
    """get_indice_pairs on coordinates that come straight from grid_unique reuses the unique's cell bitmap
    (ococc_subm_rulebook_build_sorted); it must produce the same rulebook as the generic build, in both the
    exactly-sized and the fixed-capacity (static) forms."""
    from objectcentricocccompletion_amd.spconv import ops
    from objectcentricocccompletion_amd.voxel.scatter_points import grid_unique
    g = torch.Generator().manual_seed(11)
    B, shape = 3, [12, 10, 14]
    coors = torch.stack([torch.randint(0, B, (4000,), generator=g)] +
                        [torch.randint(0, s, (4000,), generator=g) for s in shape], 1).int().to(dev)
    uc, _, _ = grid_unique(coors, [B] + shape)
    assert hasattr(uc, '_ococc_grid')
    _, p_fast, n_fast = ops.get_indice_pairs(uc, B, shape, 3, subm=True)
    _, p_ref, n_ref = ops.get_indice_pairs(uc.clone(), B, shape, 3, subm=True)   # clone: no tag -> generic path
    assert torch.equal(n_fast, n_ref) and torch.equal(p_fast, p_ref)
    assert torch.equal(p_fast._ococc.tables[(False, 'fwd')][0], p_ref._ococc.tables[(False, 'fwd')][0])
    assert torch.equal(p_fast._ococc.tables[(False, 'fwd')][1], p_ref._ococc.tables[(False, 'fwd')][1])
    us, _, _, meta = grid_unique(coors, [B] + shape, static=True)
    m = int(meta[0])
    _, p_s, n_s = ops.get_indice_pairs(us, B, shape, 3, subm=True)
    assert torch.equal(n_s, n_ref)
    for k in range(27):
        c = int(n_ref[k])
        assert torch.equal(p_s[k, :, :c], p_ref[k, :, :c])   # (past indice_num the fixed-capacity form leaves the lists unwritten)
    assert bool((p_s._ococc.tables[(False, 'fwd')][0][:, m:] == -1).all())


@pytest.mark.parametrize('cin,cout', [(16, 32), (32, 64), (64, 128), (64, 32)])
def test_fused_conv_ln_gelu_matches_unfused(dev, cin, cout):
    """make_sparse_convmodule(SubMConv3d -> LN -> GELU) with the norm in the conv epilogue
    (ococc_sparse_conv_gather_gemm_bf16 with its LayerNorm epilogue) against the same block run op by op."""
    from objectcentricocccompletion_amd.sparse_block import make_sparse_convmodule
    from objectcentricocccompletion_amd.spconv import SparseConvTensor
    from objectcentricocccompletion_amd.spconv import modules as spm
    g = torch.Generator().manual_seed(cin + cout)
    B, shape, n = 2, [10, 12, 9], 900
    cells = torch.stack([torch.randperm(10 * 12 * 9, generator=g)[:n].sort().values + b * 1080 for b in range(B)]).flatten()
    idx = torch.stack([cells // 1080, (cells // 108) % 10, (cells // 9) % 12, cells % 9], 1).int().to(dev)
    block = make_sparse_convmodule(cin, cout, 3, 'k', padding=1, conv_type='SubMConv3d', act_type='gelu',
                                   norm_cfg=dict(type='LN', eps=1e-3)).to(dev)
    with torch.no_grad():
        block[1].weight.uniform_(0.5, 1.5, generator=None)
        block[1].bias.uniform_(-0.5, 0.5)
    feats = torch.randn(idx.shape[0], cin, generator=g).to(dev).bfloat16()
    dout = torch.randn(idx.shape[0], cout, generator=g).to(dev).bfloat16()
    res = []
    for fused in (True, False):
        orig, orig_tile = spm.FUSE_CONV_LN, spm.FUSE_TILE_CONV_LN
        spm.FUSE_CONV_LN = spm.FUSE_TILE_CONV_LN = fused
        try:
            x = feats.clone().requires_grad_(True)
            block.zero_grad(set_to_none=True)
            y = block(SparseConvTensor(x, idx, shape, B)).features
            y.backward(dout)
            res.append((y.detach().float(), x.grad.float(), [p.grad.float().clone() for p in block.parameters()]))
        finally:
            spm.FUSE_CONV_LN, spm.FUSE_TILE_CONV_LN = orig, orig_tile
    (yf, gxf, gpf), (yu, gxu, gpu) = res
    assert float((yf - yu).abs().max()) <= 2e-2 * float(yu.abs().max())      # bf16 outputs: <= 1-2 ulp apart
    assert float((yf - yu).abs().mean()) <= 1e-3 * float(yu.abs().max())
    assert float((gxf - gxu).abs().max()) <= 2e-2 * float(gxu.abs().max())
    for a, b in zip(gpf, gpu):
        assert float((a - b).abs().max()) <= 2e-2 * float(b.abs().max()) + 1e-6


# ---------------------------------------------------------------- vectors from the reference's own geometry.h
def _golden_rulebook(golden_dir, name):
    import os
    g = np.load(os.path.join(golden_dir, 'rulebook.npz'))
    idx, num = g[name + '_indices'], g[name + '_num']
    pairs = np.full((len(num), 2, len(idx)), -1, np.int32)
    o = 0
    for k, c in enumerate(num):
        pairs[k, 0, :c] = g[name + '_pairs_in'][o:o + c]
        pairs[k, 1, :c] = g[name + '_pairs_out'][o:o + c]
        o += c
    return g, idx, pairs, num


@pytest.mark.parametrize('name', ['bench40', 'bench80', 'shuffled', 'dilated', 'k133'])
def test_subm_rulebook_equals_reference_geometry_h(dev, golden_dir, name):
    """ops.get_indice_pairs(subm=True) == spconv::getIndicePairsSubM (geometry.h:247-297, compiled from the
    reference by oracle/Makefile; tests/golden/rulebook.npz): counts, pairs, pair ORDER and the -1 fill."""
    from objectcentricocccompletion_amd.spconv import ops
    g, idx, ep, en = _golden_rulebook(golden_dir, name)
    outids, pairs, num = ops.get_indice_pairs(torch.from_numpy(idx).to(dev), int(g[name + '_batch']),
                                              g[name + '_shape'].tolist(), g[name + '_ksize'].tolist(), 1, 0,
                                              g[name + '_dilation'].tolist(), 0, subm=True)
    assert np.array_equal(num.cpu().numpy(), en)
    assert np.array_equal(pairs.cpu().numpy(), ep)
    assert torch.equal(outids.cpu(), torch.from_numpy(idx))


@pytest.mark.parametrize('name', ['down_k3s2p1', 'down_k2s2p0', 'down_aniso', 's1p0', 'up_k3s2p1', 'up_k2s2p0'])
def test_regular_rulebook_equals_reference_geometry_h(dev, golden_dir, name):
    """SparseConv3d / SparseConvTranspose3d rulebooks == getIndicePairsConv / DeConv (geometry.h:144-245): same
    active outputs, same pairs per offset in the same order; output rows numbered sorted (as the reference's GPU
    path does through torch::_unique, spconv_ops.h:130) instead of by first appearance (its CPU path)."""
    from objectcentricocccompletion_amd.spconv import ops
    g, idx, ep, en = _golden_rulebook(golden_dir, name)
    tr = bool(g[name + '_transpose'])
    eo = g[name + '_out_indices']
    opad = [0, 0, 0]
    if tr:  # recover the out_padding the generator used from the stored out_shape
        base = ops.get_deconv_output_size(g[name + '_shape'].tolist(), g[name + '_ksize'].tolist(),
                                          g[name + '_stride'].tolist(), g[name + '_padding'].tolist(), [1, 1, 1], opad)
        opad = [int(a - b) for a, b in zip(g[name + '_out_shape'].tolist(), base)]
    outids, pairs, num = ops.get_indice_pairs(torch.from_numpy(idx).to(dev), int(g[name + '_batch']),
                                              g[name + '_shape'].tolist(), g[name + '_ksize'].tolist(),
                                              g[name + '_stride'].tolist(), g[name + '_padding'].tolist(),
                                              g[name + '_dilation'].tolist(), opad, subm=False, transpose=tr)
    order, perm = _match_sorted(eo)
    assert np.array_equal(outids.cpu().numpy(), eo[order])
    assert np.array_equal(num.cpu().numpy(), en)
    p = pairs.cpu().numpy()
    for k in range(len(en)):
        assert np.array_equal(p[k, 0, :en[k]], ep[k, 0, :en[k]])
        assert np.array_equal(p[k, 1, :en[k]], perm[ep[k, 1, :en[k]]])
        assert (p[k, :, en[k]:] == -1).all()


@pytest.mark.parametrize('family', [None, 'sorted'])
@pytest.mark.parametrize('cin,cout', [(16, 32), (64, 128)])
@pytest.mark.parametrize('dil', [(2, 2, 2), (1, 2, 3)])
def test_dilated_subm_conv_vs_oracle(dev, dil, cin, cout, family):
    """SubMConv3d(dilation != 1): the reference keeps padding = k/2 (spconv_ops.h:66-83), so the rulebook is not
    symmetric, and indiceConv treats the offset with the most pairs as "own row" (spconv_ops.h:273-303).  Rulebook
    bit-exact, forward / dgrad / wgrad against the oracle's indiceConv restatement -- with the pattern-order switch
    forced on as well (a dilated rulebook is not its own mirror image, so ops keeps the voxel-order kernels for it
    whatever the switch says: the results must not depend on it)."""
    from objectcentricocccompletion_amd.spconv import ops
    with _kernel_family(ops, family):
        _dilated_vs_oracle(ops, dev, dil, cin, cout)


def _dilated_vs_oracle(ops, dev, dil, cin, cout):
    rng = np.random.default_rng(31)
    B, shape = 2, (9, 11, 13)
    idx = _voxels(rng, B, shape, 0.3, True)
    n = len(idx)
    _, pairs, num = ops.get_indice_pairs(torch.from_numpy(idx).to(dev), B, list(shape), 3, 1, 0, list(dil), 0, subm=True)
    ep, en = O.subm_rulebook(idx, B, shape, (3, 3, 3), dil)
    assert np.array_equal(num.cpu().numpy(), en) and np.array_equal(pairs.cpu().numpy(), ep)
    x = O.bf16_round(rng.standard_normal((n, cin)).astype(np.float32))
    w = O.bf16_round(rng.standard_normal((3, 3, 3, cin, cout)).astype(np.float32) * 0.2)
    dy = O.bf16_round(rng.standard_normal((n, cout)).astype(np.float32))
    xt, wt, dyt = (torch.from_numpy(a).to(dev) for a in (x, w, dy))
    y = ops.indice_conv(xt, wt, pairs, num, n, False, True)
    assert np.allclose(y.cpu().numpy(), O.indice_conv(x, w, ep, en, n, subm=True), **TOL)
    din, dw = ops.indice_conv_backward(xt, wt, dyt, pairs, num, False, True)
    edin, edw = O.indice_conv_backward(x, w, dy, ep, en, subm=True)
    assert np.allclose(din.cpu().numpy(), edin, **TOL)
    assert np.allclose(dw.cpu().numpy(), edw, rtol=1e-4, atol=2e-4 * max(1.0, float(np.abs(edw).max())))


# bench.py's configs[1] batch has 221 211 rulebook pairs on 126 005 rows: at that density the step runs the tile kernels
# (32 -> 64 forward with LN, both LN-backward dgrads) and the pattern-order kernel (64 -> 128 forward)
BENCH_PAIRS_PER_ROW = 1.755


@pytest.mark.parametrize('fused_front_end', [True, False])
@pytest.mark.parametrize('tile', [None, True, 'bench', 'sorted'])
def test_occupancy_encoder_vs_oracle_restatement(dev, fused_front_end, tile):
    """The configs[1] encoder end to end (voxelise -> scatter-mean -> rulebook -> 3 x (SubMConv3d, LN, GELU),
    loss = mean(out^2), backward) against oracle/encoder_ref.py, which rounds to bf16 exactly where the HIP path stores
    bf16: voxel rows bit-exact; features well inside north_star's 1e-3 (norm-wise 5e-4; the largest single deviation
    no more than one bf16 step of the largest value -- what a different f32 summation order can flip; measured 3e-5
    .. 1e-4 and 4e-4 .. 2e-3); every parameter gradient within 2e-4 (measured <= 4e-5)."""
    from objectcentricocccompletion_amd.occ_encoder import SubMOccEncoder, synthetic_object_grids
    from objectcentricocccompletion_amd.spconv import ops
    from oracle.encoder_ref import encoder_forward_backward
    torch.manual_seed(0)
    B, P = 6, 700
    xyz, feats, bidx = synthetic_object_grids(B, P, seed=3, device=dev)
    model = SubMOccEncoder(fused_front_end=fused_front_end).to(dev)
    with torch.no_grad():   # LayerNorm parameters away from (1, 0), so that their gradients are exercised
        for l in model.conv_layers:
            l[1].weight.add_(0.2 * torch.randn_like(l[1].weight))
            l[1].bias.add_(0.1 * torch.randn_like(l[1].bias))
    keep = ops.SPARSE_TILE_CONV, ops.DEFAULT_PAIRS_PER_ROW, ops.SORTED_CONV
    before = collections.Counter(ops.launches)
    if tile == 'bench':      # the kernel mix of the benchmark step: chosen by ops from the benchmark's density
        ops.DEFAULT_PAIRS_PER_ROW = BENCH_PAIRS_PER_ROW
    elif tile == 'sorted':   # every layer the pattern order is instantiated for runs on it
        ops.SORTED_CONV, ops.SPARSE_TILE_CONV = True, False
    else:
        ops.SPARSE_TILE_CONV = tile
    try:
        out = model(xyz, feats, bidx, B)
        out.features.float().pow(2).mean().backward()
    finally:
        ops.SPARSE_TILE_CONV, ops.DEFAULT_PAIRS_PER_ROW, ops.SORTED_CONV = keep
    torch.cuda.synchronize()
    ran = ops.launches - before
    if tile == 'bench':
        assert ran['sorted_ln'] >= 1 and ran['tile_ln'] + ran['tile'] >= 1, dict(ran)   # (64 -> 128 forward with its LN + GELU: round 6)
    elif tile == 'sorted':
        assert ran['sorted'] + ran['sorted_ln'] + ran['sorted_lnbwd'] >= 3 and ran['sorted_ln'] >= 1 and ran['tile'] + ran['tile_ln'] + ran['tile_lnbwd'] == 0, dict(ran)
    elif tile is None:
        assert ran['sorted'] + ran['sorted_ln'] + ran['sorted_lnbwd'] == 0, dict(ran)
    ws = [l[0].weight.detach().cpu().numpy() for l in model.conv_layers]
    gs = [l[1].weight.detach().cpu().numpy() for l in model.conv_layers]
    bs = [l[1].bias.detach().cpu().numpy() for l in model.conv_layers]
    ref = encoder_forward_backward(xyz.cpu().numpy(), feats.cpu().numpy(), bidx.cpu().numpy(), B, ws, gs, bs)
    assert np.array_equal(out.indices.cpu().numpy(), ref['vcoors'])
    got = out.features.detach().float().cpu().numpy().astype(np.float64)
    exp = ref['out'].astype(np.float64)
    assert np.linalg.norm(got - exp) <= 5e-4 * np.linalg.norm(exp)
    assert np.abs(got - exp).max() <= 2.0 ** -8 * np.abs(exp).max()
    for li, layer in enumerate(model.conv_layers):
        for name, g, e in (('dW', layer[0].weight.grad, ref['grads'][li][0]), ('dgamma', layer[1].weight.grad, ref['grads'][li][1]),
                           ('dbeta', layer[1].bias.grad, ref['grads'][li][2])):
            g = g.cpu().numpy().astype(np.float64)
            assert np.abs(g - e).max() <= 2e-4 * np.abs(e).max(), (li, name, np.abs(g - e).max() / np.abs(e).max())


@pytest.mark.parametrize('cin,cout', [(192, 64), (64, 320), (256, 144)])
def test_wide_channels_run_as_panels_vs_oracle(dev, cin, cout):
    """More than 128 input or output channels (the reference's indiceConv has no limit): contraction and columns in
    128-wide panels, same bar against the oracle; module level too (autograd through SubMConv3d)."""
    from objectcentricocccompletion_amd.spconv import SparseConvTensor, SubMConv3d, ops
    rng = np.random.default_rng(cin + cout)
    idx, x, w, dy, pairs, num, ep, en = _conv_case(rng, dev, 2, (10, 11, 12), 0.15, cin, cout)
    n = len(idx)
    xt, wt, dyt = (torch.from_numpy(a).to(dev) for a in (x, w, dy))
    y = ops.indice_conv(xt, wt, pairs, num, n, False, True)
    assert np.allclose(y.cpu().numpy(), O.indice_conv(x, w, ep, en, n, subm=True), rtol=1e-4, atol=5e-4)
    din, dw = ops.indice_conv_backward(xt, wt, dyt, pairs, num, False, True)
    edin, edw = O.indice_conv_backward(x, w, dy, ep, en, subm=True)
    assert np.allclose(din.cpu().numpy(), edin, rtol=1e-4, atol=5e-4)
    assert np.allclose(dw.cpu().numpy(), edw, rtol=1e-4, atol=2e-4 * max(1.0, float(np.abs(edw).max())))
    conv = SubMConv3d(cin, cout, 3, padding=1, bias=False, indice_key='w').to(dev)
    with torch.no_grad():
        conv.weight.copy_(wt)
    xin = xt.clone().requires_grad_(True)
    out = conv(SparseConvTensor(xin, torch.from_numpy(idx).to(dev), [10, 11, 12], 2)).features
    out.backward(dyt)
    assert np.allclose(out.detach().cpu().numpy(), y.cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert np.allclose(xin.grad.cpu().numpy(), din.cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert np.allclose(conv.weight.grad.cpu().numpy(), dw.cpu().numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('ksize', [(5, 5, 5), (1, 7, 7), (3, 3, 5)])
def test_kernel_volumes_above_32_offsets_vs_oracle(dev, ksize):
    """125, 49 and 45 offsets: the kernels walk at most 32 per launch (one mask word per 16-row block), so the offsets go
    through in slices whose f32 partial outputs are summed (spconv/ops.py:_gather_gemm); rulebook, forward, input and
    weight gradients against the oracle.  (The reference's indiceConv takes any kernel size, spconv_ops.h:300-354.)"""
    from objectcentricocccompletion_amd.spconv import ops
    rng = np.random.default_rng(sum(ksize))
    B, shape, cin, cout = 2, (12, 13, 14), 16, 32
    idx = _voxels(rng, B, shape, 0.2, True)
    n = len(idx)
    x = O.bf16_round(rng.standard_normal((n, cin)).astype(np.float32))
    w = O.bf16_round(rng.standard_normal(ksize + (cin, cout)).astype(np.float32) * 0.2)
    dy = O.bf16_round(rng.standard_normal((n, cout)).astype(np.float32))
    _, pairs, num = ops.get_indice_pairs(torch.from_numpy(idx).to(dev), B, list(shape), list(ksize), subm=True)
    ep, en = O.subm_rulebook(idx, B, shape, ksize=ksize)
    assert np.array_equal(num.cpu().numpy(), en)
    xt, wt, dyt = (torch.from_numpy(a).to(dev) for a in (x, w, dy))
    y = ops.indice_conv(xt, wt, pairs, num, n, False, True)
    assert np.allclose(y.cpu().numpy(), O.indice_conv(x, w, ep, en, n, subm=True), **TOL)
    yb = ops.indice_conv(xt.bfloat16(), wt.bfloat16(), pairs, num, n, False, True)
    assert yb.dtype == torch.bfloat16 and torch.equal(yb, y.bfloat16())
    din, dw = ops.indice_conv_backward(xt, wt, dyt, pairs, num, False, True)
    edin, edw = O.indice_conv_backward(x, w, dy, ep, en, subm=True)
    assert np.allclose(din.cpu().numpy(), edin, **TOL)
    assert np.allclose(dw.cpu().numpy(), edw, rtol=1e-4, atol=2e-4 * max(1.0, float(np.abs(edw).max())))


def test_transposed_and_2d_modules_vs_dense(dev):
    """SparseConvTranspose3d / SparseConvTranspose2d (conv.py:286-337 of the reference) against torch's dense transposed
    convolution on the scattered volume (every output site the dense result is non-zero at is an output row; equal
    values there), SparseConv2d + SparseInverseConv2d (conv.py:340-356) returning to the input sites; gradients exist."""
    from objectcentricocccompletion_amd.spconv import (SparseConv2d, SparseConvTensor, SparseConvTranspose2d,
                                                       SparseConvTranspose3d, SparseInverseConv2d)
    rng = np.random.default_rng(31)
    torch.manual_seed(2)
    for ndim, shape, cls in ((3, (5, 6, 7), SparseConvTranspose3d), (2, (9, 11), SparseConvTranspose2d)):
        B, cin, cout = 2, 16, 32
        idx = _voxels(rng, B, shape, 0.25, True)
        n = len(idx)
        layer = cls(cin, cout, 3, stride=2, padding=1, bias=False).to(dev)
        x = O.bf16_round(rng.standard_normal((n, cin)).astype(np.float32))
        xt = torch.from_numpy(x).to(dev).requires_grad_(True)
        out = layer(SparseConvTensor(xt, torch.from_numpy(idx).to(dev), list(shape), B))
        w = torch.from_numpy(O.bf16_round(layer.weight.detach().cpu().numpy()))
        dense = torch.zeros((B,) + shape + (cin,))
        dense[tuple(idx[:, i] for i in range(ndim + 1))] = torch.from_numpy(x)
        if ndim == 3:
            # weight [kD,kH,kW,Cin,Cout] -> conv_transpose3d's [Cin, Cout, kD, kH, kW]
            yd = torch.nn.functional.conv_transpose3d(dense.permute(0, 4, 1, 2, 3), w.permute(3, 4, 0, 1, 2), stride=2,
                                                      padding=1).permute(0, 2, 3, 4, 1)
        else:
            yd = torch.nn.functional.conv_transpose2d(dense.permute(0, 3, 1, 2), w.permute(2, 3, 0, 1), stride=2,
                                                      padding=1).permute(0, 2, 3, 1)
        assert list(out.spatial_shape) == list(yd.shape[1:-1])
        oi = out.indices.cpu().numpy()
        got = out.features.detach().float().cpu().numpy()
        assert np.allclose(got, yd[tuple(oi[:, i] for i in range(ndim + 1))].numpy(), rtol=1e-3, atol=2e-3)
        covered = torch.zeros(yd.shape[:-1], dtype=torch.bool)
        covered[tuple(oi[:, i] for i in range(ndim + 1))] = True
        assert float(yd[~covered].abs().max()) == 0.0 if bool((~covered).any()) else True
        out.features.float().pow(2).sum().backward()
        assert bool(torch.isfinite(xt.grad).all()) and float(xt.grad.abs().sum()) > 0 and layer.weight.grad is not None
    # 2-D strided conv and its inverse partner
    B, shape, cin, cmid = 2, (12, 14), 16, 32
    idx = _voxels(rng, B, shape, 0.3, True)
    n = len(idx)
    down = SparseConv2d(cin, cmid, 3, stride=2, padding=1, bias=False, indice_key='p').to(dev)
    up = SparseInverseConv2d(cmid, cin, 3, indice_key='p', bias=False).to(dev)
    xt = torch.from_numpy(O.bf16_round(rng.standard_normal((n, cin)).astype(np.float32))).to(dev).requires_grad_(True)
    mid = down(SparseConvTensor(xt, torch.from_numpy(idx).to(dev), list(shape), B))
    out = up(mid)
    assert out.features.shape == (n, cin) and torch.equal(out.indices.cpu(), torch.from_numpy(idx))
    dense = torch.zeros((B,) + shape + (cin,))
    dense[idx[:, 0], idx[:, 1], idx[:, 2]] = xt.detach().cpu()
    w1 = torch.from_numpy(O.bf16_round(down.weight.detach().cpu().numpy()))
    yd = torch.nn.functional.conv2d(dense.permute(0, 3, 1, 2), w1.permute(3, 2, 0, 1), padding=1, stride=2).permute(0, 2, 3, 1)
    oi = mid.indices.cpu().numpy()
    assert np.allclose(mid.features.detach().float().cpu().numpy(), yd[oi[:, 0], oi[:, 1], oi[:, 2]].numpy(), rtol=1e-3, atol=2e-3)
    out.features.float().pow(2).sum().backward()
    assert bool(torch.isfinite(xt.grad).all()) and up.weight.grad is not None and down.weight.grad is not None


def test_sparse_bottleneck_block_vs_dense_math(dev):
    """SparseBottleneck (sparse_block.py:22-78): 1x1 -> BN -> ReLU -> 3x3 sub-manifold -> BN -> ReLU -> 1x1 -> BN, + identity,
    ReLU -- against the same chain written with the oracle's sub-manifold convolution and torch's batch norm (eval)."""
    from objectcentricocccompletion_amd.sparse_block import SparseBottleneck
    from objectcentricocccompletion_amd.spconv import SparseConvTensor
    rng = np.random.default_rng(41)
    torch.manual_seed(4)
    B, shape, planes = 2, (9, 10, 11), 16
    idx = _voxels(rng, B, shape, 0.25, True)
    n = len(idx)
    blk = SparseBottleneck(planes * 4, planes, conv_cfg=dict(type='SubMConv3d', indice_key='b'), norm_cfg=dict(type='BN1d')).to(dev).eval()
    with torch.no_grad():
        for bn in (blk.norm1, blk.norm2, blk.norm3):
            bn.running_mean.normal_(0, 0.1)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.1)
    x = rng.standard_normal((n, planes * 4)).astype(np.float32)
    out = blk(SparseConvTensor(torch.from_numpy(x).to(dev), torch.from_numpy(idx).to(dev), list(shape), B))
    ep, en = O.subm_rulebook(idx, B, shape)
    bnf = lambda bn, v: torch.nn.functional.batch_norm(torch.from_numpy(v), bn.running_mean.cpu(), bn.running_var.cpu(),
                                                       bn.weight.detach().cpu(), bn.bias.detach().cpu(), False, 0.0, bn.eps).numpy()
    w1, w2, w3 = (c.weight.detach().cpu().numpy() for c in (blk.conv1, blk.conv2, blk.conv3))
    h = np.maximum(bnf(blk.norm1, x @ w1.reshape(planes * 4, planes)), 0)
    h = np.maximum(bnf(blk.norm2, O.indice_conv(O.bf16_round(h), O.bf16_round(w2), ep, en, n, subm=True)), 0)
    want = np.maximum(bnf(blk.norm3, h @ w3.reshape(planes, planes * 4)) + x, 0)
    got = out.features.detach().float().cpu().numpy()
    assert got.shape == want.shape and float(np.abs(got - want).max()) < 2e-2 * max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_sparse_maxpool_vs_oracle_and_dense(dev, dtype):
    """SparseMaxPool3d (pool.py:20-87) / indice_maxpool(_backward) (ops.py:162-184): forward and input gradient bit for
    bit against the restatement of the reference's CPU functor (output starting at ZERO, the gradient to every input
    equal to the maximum, offsets ascending), and -- on positive inputs -- against torch's dense max_pool3d."""
    from objectcentricocccompletion_amd.spconv import SparseConvTensor, SparseMaxPool3d, ops
    rng = np.random.default_rng(51)
    B, shape, c = 2, (9, 10, 12), 16
    idx = _voxels(rng, B, shape, 0.3, True)
    n = len(idx)
    x = O.bf16_round(rng.standard_normal((n, c)).astype(np.float32))
    x[rng.random(x.shape) < 0.1] = 0.0                                   # ties with the zero start and among inputs
    x[1::7] = x[0::7][:len(x[1::7])]
    xt = torch.from_numpy(x).to(dev).to(dtype).requires_grad_(True)
    pool = SparseMaxPool3d(3, stride=2, padding=1)
    out = pool(SparseConvTensor(xt, torch.from_numpy(idx).to(dev), list(shape), B))
    oshape = [(s + 2 - 3) // 2 + 1 for s in shape]
    assert list(out.spatial_shape) == oshape
    eo, ep, en = O.conv_rulebook(idx, B, oshape, (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1))
    order, _ = _match_sorted(eo)
    want = O.indice_maxpool(x, ep, en, len(eo))
    got = out.features.detach().float().cpu().numpy()
    assert np.array_equal(got, want[order])
    dy = O.bf16_round(rng.standard_normal(want.shape).astype(np.float32))
    dyt = torch.from_numpy(dy[order]).to(dev).to(dtype)
    out.features.backward(dyt)
    edin = O.indice_maxpool_backward(x, want, dy, ep, en)
    gin = xt.grad.float().cpu().numpy()
    if dtype == torch.float32:
        assert np.array_equal(gin, edin)
    else:
        assert np.allclose(gin, edin, rtol=1e-2, atol=1e-2)            # (the sum over offsets is rounded to bf16)
    # dense cross-check on positive features (zero start = the dense pool's implicit padding then)
    xp = np.abs(x) + 0.5
    dense = torch.zeros((B, c) + shape)
    dense[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]] = torch.from_numpy(xp)
    yd = torch.nn.functional.max_pool3d(dense, 3, stride=2, padding=1)
    outp = pool(SparseConvTensor(torch.from_numpy(xp).to(dev).to(dtype), torch.from_numpy(idx).to(dev), list(shape), B))
    oi = outp.indices.cpu().numpy()
    ref = yd[oi[:, 0], :, oi[:, 1], oi[:, 2], oi[:, 3]].to(dtype).float().numpy()
    assert np.array_equal(outp.features.float().cpu().numpy(), ref)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_submanifold_maxpool_and_half_precision(dev, dtype):
    """SparseMaxPool(subm=True) (pool.py:20-87 with the sub-manifold rulebook: the output keeps the input's sites) and the
    reference's half instantiation (indice_maxpool_half, ops.py:162-184): forward and input gradient bit for bit against the
    restatement of the CPU functor on the oracle's sub-manifold rulebook (this path was unexercised; the
    backward derives its table from saved pairs that were built without -1 tails)."""
    from objectcentricocccompletion_amd.spconv import SparseConvTensor, ops
    from objectcentricocccompletion_amd.spconv.pool import SparseMaxPool
    rng = np.random.default_rng(52)
    B, shape, c = 2, (9, 10, 12), 16
    idx = _voxels(rng, B, shape, 0.3, False)
    n = len(idx)
    x = rng.standard_normal((n, c)).astype(np.float16).astype(np.float32)      # f16-representable values
    x[rng.random(x.shape) < 0.1] = 0.0
    xt = torch.from_numpy(x).to(dev).to(dtype).requires_grad_(True)
    pool = SparseMaxPool(3, 3, stride=1, padding=1, subm=True)
    out = pool(SparseConvTensor(xt, torch.from_numpy(idx).to(dev), list(shape), B))
    assert torch.equal(out.indices.cpu(), torch.from_numpy(idx)) and out.features.dtype == dtype
    ep, en = O.subm_rulebook(idx, B, shape)
    want = O.indice_maxpool(x, ep, en, n)
    assert np.array_equal(out.features.detach().float().cpu().numpy(), want)
    dy = rng.standard_normal(want.shape).astype(np.float16).astype(np.float32)
    out.features.backward(torch.from_numpy(dy).to(dev).to(dtype))
    edin = O.indice_maxpool_backward(x, want, dy, ep, en)
    gin = xt.grad.float().cpu().numpy()
    if dtype == torch.float32:
        assert np.array_equal(gin, edin)
    else:
        assert np.allclose(gin, edin, rtol=2e-3, atol=2e-3)                   # (the sum over offsets is rounded to f16)


def test_sequential_fused_folds_batchnorm_into_the_conv(dev):
    """SparseSequential.fused() (modules.py:139-185): conv + BatchNorm1d folded into one conv with a bias (the
    reference's arithmetic, whose denominator is sqrt(var) + eps); equal to the unfused eval-mode chain to that
    difference."""
    from objectcentricocccompletion_amd.spconv import SparseConvTensor, SparseSequential, SubMConv3d
    rng = np.random.default_rng(61)
    torch.manual_seed(6)
    B, shape = 2, (8, 9, 10)
    idx = _voxels(rng, B, shape, 0.3, True)
    seq = SparseSequential(SubMConv3d(16, 32, 3, padding=1, bias=False, indice_key='s'), torch.nn.BatchNorm1d(32),
                           torch.nn.ReLU()).to(dev).eval()
    with torch.no_grad():
        seq[1].running_mean.normal_(0, 0.2)
        seq[1].running_var.uniform_(0.5, 2.0)
        seq[1].weight.uniform_(0.5, 1.5)
        seq[1].bias.normal_(0, 0.2)
    x = torch.from_numpy(O.bf16_round(rng.standard_normal((len(idx), 16)).astype(np.float32))).to(dev)
    mk = lambda: SparseConvTensor(x.clone(), torch.from_numpy(idx).to(dev), list(shape), B)
    fused = seq.fused().eval()
    assert len(fused) == 2 and fused[0].fused_bn and fused[0].bias is not None
    with torch.no_grad():
        a, b = seq(mk()).features, fused(mk()).features
    assert float((a - b).abs().max()) < 2e-2 * float(a.abs().max())


def test_adaptive_sparse_basic_block_runs_on_strided_sites(dev):
    """AdaptiveSparseBasicBlock (sparse_block.py:146-213): the strided adaptive conv moves the tensor to the coarser
    sites, the basic block keeps them; forward / backward finite, output sites = those of the strided rulebook."""
    from objectcentricocccompletion_amd.sparse_block import AdaptiveSparseBasicBlock
    from objectcentricocccompletion_amd.spconv import SparseConvTensor, ops
    rng = np.random.default_rng(71)
    torch.manual_seed(7)
    B, shape = 2, (8, 10, 12)
    idx = _voxels(rng, B, shape, 0.3, True)
    blk = AdaptiveSparseBasicBlock(16, 32, stride=2, conv_cfg=dict(type='SubMConv3d', indice_key='a'),
                                   norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01)).to(dev).train()
    x = torch.randn(len(idx), 16, device=dev, requires_grad=True)
    out = blk(SparseConvTensor(x, torch.from_numpy(idx).to(dev), list(shape), B))
    want_ids, _, _ = ops.get_indice_pairs(torch.from_numpy(idx).to(dev), B, list(shape), [2, 2, 2], [2, 2, 2], [0, 0, 0])
    assert list(out.spatial_shape) == [4, 5, 6] and torch.equal(out.indices, want_ids) and out.features.shape[1] == 32
    out.features.pow(2).sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().sum()) > 0
