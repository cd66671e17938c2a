"""linear.rows_wgrad / linear.wgrad_rows_bf16 / linear.mm_f32 on the device against the expressions they replaced
(test_rows_wgrad_cpu.py keeps them as they stood): the same library calls on the same shapes, so the results are compared
with torch.equal.  Where the library itself does not repeat its own bits from one call to the next (checked first, per
shape), both are held against a float64 contraction instead and the helper may not be further off than the parent
expression was in either of its two evaluations."""
import pytest
import torch

from test_rows_wgrad_cpu import frozen_height_rule, frozen_qkv_slabs, frozen_slices32_f32, frozen_token_slabs, operands

pytestmark = pytest.mark.gpu


def _same_as_parent(got, parent, exact):
    """``parent`` / ``exact``: callables (the frozen expression, the float64 contraction)"""
    ref, again = parent(), parent()
    assert got.dtype == ref.dtype == torch.float32 and got.shape == ref.shape
    if torch.equal(ref, again):
        assert torch.equal(got, ref)
        return
    e = exact()
    errs = [float((t.double() - e).abs().max()) for t in (got, ref, again)]
    print('library not bit-reproducible for this shape: max |error| helper %.3e, parent %.3e / %.3e' % tuple(errs))
    assert errs[0] <= max(errs[1:])


# 511 rows per slice (one product), 512, 512 + a remainder; 1 output column is padded to 16; 8 input columns: one product
@pytest.mark.parametrize('cin', [8, 64])
@pytest.mark.parametrize('cout', [1, 16, 64])
@pytest.mark.parametrize('rows', [16352, 16384, 16461])
def test_32_slices_f32_partials_equal_the_parent_expression(dev, rows, cout, cin):
    from objectcentricocccompletion_amd import linear
    dz, y = operands(rows, cout, cin, torch.bfloat16, dev)
    _same_as_parent(linear.wgrad_rows_bf16(dz, y), lambda: frozen_slices32_f32(dz, y), lambda: dz.double().t() @ y.double())


def test_height_rule_and_64_slabs_on_the_device_equal_the_parent_expressions(dev):
    from objectcentricocccompletion_amd import linear
    gy, x = operands(20557, 40, 24, torch.float32, dev)
    _same_as_parent(linear.rows_wgrad(gy, x), lambda: frozen_height_rule(gy, x), lambda: gy.double().t() @ x.double())
    dy, t = operands(6405, 32, 16, torch.bfloat16, dev)
    _same_as_parent(linear.rows_wgrad(dy, t, slices=64), lambda: frozen_token_slabs(dy, t), lambda: dy.double().t() @ t.double())
    E = 16
    g, v = operands(1000, 3 * E, E, torch.bfloat16, dev)
    vp = v + operands(1000, 1, E, torch.bfloat16, dev)[1]
    got = torch.cat([linear.rows_wgrad(g[:, :2 * E], vp, slices=64), linear.rows_wgrad(g[:, 2 * E:], v, slices=64)], 0)
    _same_as_parent(got, lambda: frozen_qkv_slabs(g, vp, v),
                    lambda: torch.cat([g[:, :2 * E].double().t() @ vp.double(), g[:, 2 * E:].double().t() @ v.double()], 0))


def test_mm_f32_of_bf16_operands_is_as_close_to_float64_as_the_parent_helper(dev):
    """bf16 [300, 128] @ [128, 128] -> f32 without a rounding in between: no further from the float64 product than
    sst_modules._mm_f32 (torch.mm of the contiguous operands with out_dtype) was on the same inputs."""
    from objectcentricocccompletion_amd import linear
    a, b = operands(128, 300, 128, torch.bfloat16, dev)
    a = a.t().contiguous()                                                     # [300, 128]
    exact = a.double() @ b.double()
    parent = torch.mm(a.contiguous(), b.contiguous(), out_dtype=torch.float32)
    got = linear.mm_f32(a, b)
    assert got.dtype == torch.float32
    err, parent_err = float((got.double() - exact).abs().max()), float((parent.double() - exact).abs().max())
    print('mm_f32 max |error| %.3e, parent %.3e' % (err, parent_err))
    assert err <= parent_err
