"""nn.Linear for the per-point layers of the RoI encoder (same parameters, same state-dict keys), and the row-sliced
weight gradient that every tall Linear of the package uses.

The SIR layers and their MLPs (voxel_encoder.py:686-832, sst_ops.py:333-360) apply Linear(16..144 -> 3..144) to every
point of the batch: 1.3e5 rows at 64 tracklets.  Their weight gradient dW = dY^T X is then a GEMM with a tiny output and
a contraction 1e5 long, which the library runs as a handful of macro tiles (47 such GEMMs = 19 ms of a 157 ms step);
rows_wgrad below cuts it into slices.  Forward and input gradient are the ordinary GEMMs."""
import os

import torch
import torch.nn.functional as F
from torch import nn

TALL_ROWS = int(os.environ.get('OCOCC_TALL_ROWS', 16384))   # from this many rows on (and <= 256 features) the sliced weight gradient is used
POINT_TALL_ROWS = 4096   # point_mlp.weight_grad's library path: lower since the slice height adapts (4096 rows = 16 slices of 256), not tied to Linear's dispatch


def _op(a):
    return torch.bmm if a.dim() == 3 else torch.mm


def mm_f32(a, b):
    """a @ b (2-D or batched) with an f32 result: f32 operands as they are; bf16 operands on the device with f32
    accumulation and no rounding of the result (out_dtype), on the CPU through f32 copies of the operands."""
    if a.dtype == torch.float32:
        return _op(a)(a, b)
    if a.is_cuda:
        return _op(a)(a, b, out_dtype=torch.float32)
    return _op(a)(a.float(), b.float())


def rows_wgrad(gy, x, height=None, slices=None, f32_partials=False):
    """dY^T X -> f32 [out, in] for gy [n, out], x [n, in] (column-slice views allowed, nothing is copied): the rows are
    cut into ``slices`` slices or into slices of ``height`` rows (default: 4096 rows, less for inputs of a few 1e4 rows so
    that the batched GEMM still has ~64 slices to spread over the chip), the slices contracted as ONE batched GEMM, the partial
    products summed in f32 in a fixed order and the remainder rows added as one more product.  Partial products: in the
    operand dtype, or with ``f32_partials`` (bf16 operands, device only) in f32 without a rounding.  As ONE GEMM the
    library runs the small [out, in] result as a few macro tiles over the whole contraction.  Measured on MI355X:

    call sites                               slicing                 one GEMM -> sliced           probe (tools/probe/)
    _TallLinear (1.3e5 rows, <= 144 wide),   height rule, f32        340-380 us -> 35-65 us;      tall_wgrad.py
      _TallAddmm, decoder first layer                                60 -> 512 at 1 M: 2.3 ms one
      (60 -> 512, 1 M rows), point_mlp                               tile; 8 slices of 33 k rows
                                                                     49 us, hence ~64 slices
    decoder backward, _MixedLinear           32 slices, f32 partials 1024 x 1024 at 1 M rows      dec_gemm_bench.py,
      (wgrad_rows_bf16)                      (not rounded to bf16)   4.1 -> 2.05 ms, 1024 x 512   bmm_host_probe.py
                                                                     3.4 -> 1.08 ms
    _TokenLinear, _QkvProjection             64 slabs, bf16 partials a dozen workgroups, ~0.6 ms  --
      (~1e5..1e6 tokens, E x E)                                      -> thousands of tiles"""
    n = gy.shape[0]
    if height is None:
        height = min(4096, max(256, (n // 64) // 256 * 256))
    per, s = (n // slices, slices) if slices else (height, n // height)
    main = per * s
    mm = mm_f32 if f32_partials else (lambda a, b: _op(a)(a, b))
    out = None
    if main:
        out = mm(gy[:main].unflatten(0, (s, per)).transpose(1, 2), x[:main].unflatten(0, (s, per))).float().sum(0)
    if out is None or main < n:
        tail = mm(gy[main:].t(), x[main:]).float()
        out = tail if out is None else out + tail
    return out


def wgrad_rows_bf16(dz, y):
    """rows_wgrad for bf16 dz [M, n], y [M, k] on the device, M in the 1e5..1e6: 32 slices, f32 partial products."""
    M, n = dz.shape
    if M // 32 < 512 or y.shape[1] < 16:
        return (dz.t() @ y).float()
    if n < 16:   # (the head's 1-wide gradient: as it is, the batched form takes a path that costs 11 ms of HOST time per call;
        wide = torch.zeros((M, 16), dtype=dz.dtype, device=dz.device)   # padded to 16 columns it is the fast one -- 1.4 ms
        wide[:, :n] = dz                                               # less per 64-tracklet step than one skinny GEMM)
        return wgrad_rows_bf16(wide, y)[:n]
    return rows_wgrad(dz, y, slices=32, f32_partials=True)


class _TallLinear(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gy @ weight if ctx.needs_input_grad[0] else None
        gw = rows_wgrad(gy, x) if ctx.needs_input_grad[1] else None
        gb = gy.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return gx, gw, gb


class _TallAddmm(torch.autograd.Function):
    """base + x @ w^T for 1e5..1e6 rows and a small weight (the per-query half of the occupancy decoder's first layer:
    60 positional-encoding channels -> 512): the weight gradient is rows_wgrad."""

    @staticmethod
    def forward(ctx, base, x, w):
        ctx.save_for_backward(x, w)
        return torch.addmm(base, x, w.t())

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gy @ w if ctx.needs_input_grad[1] else None
        gw = rows_wgrad(gy, x).to(w.dtype) if ctx.needs_input_grad[2] else None
        return (gy if ctx.needs_input_grad[0] else None), gx, gw


def tall_addmm(base, x, w):
    """torch.addmm(base, x, w.t()) with the sliced weight gradient when there are many rows."""
    if x.dim() == 2 and x.size(0) >= TALL_ROWS and x.dtype == w.dtype == base.dtype and torch.is_grad_enabled():
        return _TallAddmm.apply(base, x.contiguous(), w)
    return torch.addmm(base, x, w.t())


class Linear(nn.Linear):

    def forward(self, x):
        from . import gemm
        if gemm.GEMM_DTYPE is not None and x.is_cuda and x.dtype == torch.float32 and min(self.in_features, self.out_features) >= 16:
            return gemm.linear(x, self.weight, self.bias)   # bf16 operands on the matrix cores, f32 sums (opt-in: gemm.py)
        if (x.dim() == 2 and x.size(0) >= TALL_ROWS and max(self.in_features, self.out_features) <= 256
                and x.dtype == torch.float32 and x.is_contiguous() and torch.is_grad_enabled()):
            return _TallLinear.apply(x, self.weight, self.bias)
        if min(self.in_features, self.out_features) >= 256 and gemm._split3_ok(x, self.weight, self.bias):
            # the RoI-level MLPs (ococc_bbox_head.py:116-193: 3072 -> 2048 -> 2048 -> 1536, ...) from a few hundred RoIs on:
            # one bf16 GEMM over three-way split operands, f32-level accuracy (gemm.py)
            return gemm.linear(x, self.weight, self.bias)
        return F.linear(x, self.weight, self.bias)
