"""linear.rows_wgrad -- the one row-sliced weight gradient dW = dY^T X of the package -- against the expressions it
replaced, kept here as they stood at their call sites: the same products summed in the same order, so the comparison is
torch.equal and not a tolerance.  (The mode the CPU cannot run, f32 partial products of bf16 operands, is in
test_gpu_rows_wgrad.py, which takes the frozen expressions from here.)"""
import pytest
import torch


def frozen_height_rule(gy, x):
    """linear.sliced_wgrad (_TallLinear, _TallAddmm, the decoder's first layer, point_mlp.weight_grad's library path)"""
    n, cout = gy.shape
    cin = x.shape[1]
    rows = min(4096, max(256, (n // 64) // 256 * 256))
    s = n // rows
    out = (gy[:s * rows].view(s, rows, cout).transpose(1, 2) @ x[:s * rows].view(s, rows, cin)).sum(0)
    if s * rows < n:
        out = out + gy[s * rows:].t() @ x[s * rows:]
    return out


def frozen_token_slabs(dy, x, s=64):
    """sst_modules._TokenLinear.backward's weight gradient"""
    n = x.shape[0]
    m = (n // s) * s
    dw = None
    if m:
        part = torch.bmm(dy[:m].view(s, m // s, -1).transpose(1, 2), x[:m].view(s, m // s, -1))
        dw = part.float().sum(0)
    if m < n:
        tail = (dy[m:].t() @ x[m:]).float()
        dw = tail if dw is None else dw + tail
    return dw


def frozen_qkv_slabs(g, xp, x, s=64):
    """sst_modules._QkvProjection.backward's weight gradient: g [V, 3E] contiguous, read through its column slices"""
    E = x.shape[1]
    g_qk, g_v = g[:, :2 * E], g[:, 2 * E:]
    n = x.shape[0]
    m = (n // s) * s
    dw = torch.zeros((3 * E, E), dtype=torch.float32, device=x.device)
    if m:
        gs = g[:m].view(s, m // s, 3 * E)
        dw[:2 * E] += torch.bmm(gs[:, :, :2 * E].transpose(1, 2), xp[:m].view(s, m // s, E)).float().sum(0)
        dw[2 * E:] += torch.bmm(gs[:, :, 2 * E:].transpose(1, 2), x[:m].view(s, m // s, E)).float().sum(0)
    if m < n:
        dw[:2 * E] += (g_qk[m:].t() @ xp[m:]).float()
        dw[2 * E:] += (g_v[m:].t() @ x[m:]).float()
    return dw


def frozen_slices32_f32(dz, y, slices=32):
    """fused_mlp.wgrad_rows_bf16 (the decoder backward's three products, gemm._MixedLinear.backward); device only"""
    M, n = dz.shape
    per = M // slices
    if per < 512 or y.shape[1] < 16:
        return (dz.t() @ y).float()
    if n < 16:
        wide = torch.zeros((M, 16), dtype=dz.dtype, device=dz.device)
        wide[:, :n] = dz
        return frozen_slices32_f32(wide, y, slices)[:n]
    main = per * slices
    out = torch.bmm(dz[:main].view(slices, per, dz.shape[1]).transpose(1, 2), y[:main].view(slices, per, y.shape[1]),
                    out_dtype=torch.float32).sum(0)
    if main < M:
        out = out + torch.mm(dz[main:].t(), y[main:], out_dtype=torch.float32)
    return out


def operands(n, cout, cin, dtype, device='cpu'):
    g = torch.Generator().manual_seed(n * 131 + cout)
    return (torch.randn(n, cout, generator=g).to(dtype).to(device), torch.randn(n, cin, generator=g).to(dtype).to(device))


@pytest.mark.parametrize('n', [100, 255, 256, 4173, 20557, 70000])   # no full slice (the remainder alone) .. 4096-row slices
def test_height_rule_f32_equals_the_parent_expression(n):
    from objectcentricocccompletion_amd import linear
    gy, x = operands(n, 40, 24, torch.float32)
    got = linear.rows_wgrad(gy, x)
    assert got.dtype == torch.float32 and got.shape == (40, 24)
    assert torch.equal(got, frozen_height_rule(gy, x))


@pytest.mark.parametrize('n', [10, 63, 64, 1000, 6405])   # fewer rows than slabs (the remainder alone), exact, remainders
def test_64_slabs_bf16_equals_the_parent_expression(n):
    from objectcentricocccompletion_amd import linear
    dy, x = operands(n, 32, 16, torch.bfloat16)
    got = linear.rows_wgrad(dy, x, slices=64)
    assert got.dtype == torch.float32 and got.shape == (32, 16)
    assert torch.equal(got, frozen_token_slabs(dy, x))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_64_slabs_over_column_slice_views_equal_the_accumulation_into_zeros(dtype):
    from objectcentricocccompletion_amd import linear
    E = 16
    g, x = operands(1000, 3 * E, E, dtype)
    xp = x + operands(1000, 1, E, dtype)[1]
    g_qk, g_v = g[:, :2 * E], g[:, 2 * E:]
    assert not g_qk.is_contiguous() and g_qk.data_ptr() == g.data_ptr()
    got = torch.cat([linear.rows_wgrad(g_qk, xp, slices=64), linear.rows_wgrad(g_v, x, slices=64)], 0)
    assert torch.equal(got, frozen_qkv_slabs(g, xp, x))


def test_mm_f32_on_the_cpu():
    """f32 operands: torch.mm / torch.bmm themselves; bf16 operands: the product of their f32 copies"""
    from objectcentricocccompletion_amd import linear
    a, b = operands(128, 300, 40, torch.float32)
    assert torch.equal(linear.mm_f32(a.t(), b), torch.mm(a.t(), b))
    a16, b16 = a.to(torch.bfloat16), b.to(torch.bfloat16)
    got = linear.mm_f32(a16.t(), b16)
    assert got.dtype == torch.float32 and torch.equal(got, a16.float().t() @ b16.float())
    a3, b3 = a16.view(4, 32, 300), b16.view(4, 32, 40)
    assert torch.equal(linear.mm_f32(a3.transpose(1, 2), b3), torch.bmm(a3.float().transpose(1, 2), b3.float()))
