"""tests/ln_ref.py, the float64 reference the LayerNorm(+GELU) kernel tests compare with, against torch's float64
autograd; and the statistics of its restatement of the dropout hash."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ln_ref as R        # noqa: E402

THR = round(0.1 * 65536)
SEED = (0x5bd1e995 << 32) | 0x1b873593     # both halves non-zero


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('act', ['none', 'gelu'])
@pytest.mark.parametrize('n,c', [(7, 5), (33, 131), (4, 1024)])
def test_ln_ref_against_float64_autograd(n, c, act, masked):
    g = torch.Generator().manual_seed(1000 * n + c)
    x = (2 * torch.randn(n, c, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    gamma = (torch.rand(c, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = (0.1 * torch.randn(c, generator=g, dtype=torch.float64)).requires_grad_(True)
    dy = torch.randn(n, c, generator=g, dtype=torch.float64) + 1
    eps = 1e-3
    keep, scale = None, 1.0
    if masked:
        keep = torch.rand(n, c, generator=g) >= 0.25
        scale = 4.0 / 3.0
    y = torch.nn.functional.layer_norm(x, (c,), gamma, beta, eps)
    if act == 'gelu':
        y = torch.nn.functional.gelu(y)
    if masked:
        y = y * keep * scale
    y.backward(dy)
    yr, mean, rstd = R.ln_act(x.detach(), gamma.detach(), beta.detach(), eps, act, keep, scale)
    dx, dg, db, adg, adb = R.ln_act_backward(x.detach(), dy, gamma.detach(), beta.detach(), eps, act, keep, scale)
    assert _close(yr, y.detach()) and _close(dx, x.grad) and _close(dg, gamma.grad) and _close(db, beta.grad)
    xd = x.detach()
    assert _close(mean, xd.mean(1)) and _close(rstd, 1 / torch.sqrt(xd.var(1, unbiased=False) + eps))
    assert bool((adg >= dg.abs()).all()) and bool((adb >= db.abs()).all())
    # the same numbers from given statistics, and as numbers of another kind when they are a little off
    again = R.ln_act_backward(xd, dy, gamma.detach(), beta.detach(), eps, act, keep, scale, stats=(mean, rstd))
    assert all(torch.equal(a, b) for a, b in zip(again, (dx, dg, db, adg, adb)))
    off = R.ln_act_backward(xd, dy, gamma.detach(), beta.detach(), eps, act, keep, scale, stats=(mean + 1e-3, rstd))
    assert not _close(off[0], dx)


def test_gelu_tails_keep_their_relative_accuracy():
    z = torch.tensor([-12.0, -6.0, -1.0, 0.0, 1.0, 6.0, 12.0], dtype=torch.float64)
    phi = torch.tensor([1.7764821120776842e-33, 9.8658764503769437e-10, 0.15865525393145707, 0.5,
                        0.84134474606854293, 0.99999999901341235, 1.0], dtype=torch.float64)
    assert float(((R.norm_cdf(z) - phi).abs() / phi).max()) < 1e-13
    assert float((R.gelu(z) - z * phi).abs().max()) < 1e-15
    h = 1e-6     # the derivative against a central difference of the value
    num = (R.gelu(z + h) - R.gelu(z - h)) / (2 * h)
    assert float((R.gelu_grad(z) - num).abs().max()) < 1e-9


def test_dropout_keep_is_a_function_of_its_arguments():
    a, b = R.dropout_keep(300, 512, THR, SEED), R.dropout_keep(300, 512, THR, SEED)
    assert a.dtype == bool and a.shape == (300, 512) and np.array_equal(a, b)
    assert not np.array_equal(a, R.dropout_keep(300, 512, THR, SEED + 1))            # low half
    assert not np.array_equal(a, R.dropout_keep(300, 512, THR, SEED + 2 ** 32))      # high half
    assert R.dropout_keep(300, 512, 0, SEED).all()                                   # threshold 0 keeps everything
    # the hash of a pair depends on row * (c / 2) + pair alone: [n, c] and [2 n, c / 2] are the same stream
    assert np.array_equal(a, R.dropout_keep(600, 256, THR, SEED).reshape(300, 512))


def test_dropout_keep_by_hand_for_one_pair():
    """row 3, pair 5 of 8 (c = 16) with Python integers"""
    row, pair, pairs, thr = 3, 5, 8, THR
    m = 0xffffffff
    h = ((row * pairs + pair) & m) ^ (SEED & m)
    h = (h * 0x9E3779B1) & m
    h ^= h >> 16
    h = ((h + (SEED >> 32) + (row >> 24)) * 0x85EBCA6B) & m
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & m
    h ^= h >> 16
    keep = R.dropout_keep(4, 16, thr, SEED)
    assert keep[3, 10] == ((h & 0xffff) >= thr) and keep[3, 11] == ((h >> 16) >= thr)


def test_dropout_keep_rate():
    n, c, p = 4096, 512, THR / 65536
    keep = R.dropout_keep(n, c, THR, SEED)
    drop = 1.0 - keep.mean()
    assert abs(drop - 0.1) < 5 * (p * (1 - p) / (n * c)) ** 0.5, drop
    per_channel = 1.0 - keep.mean(0)
    six = 6 * (p * (1 - p) / n) ** 0.5
    assert per_channel.max() < 0.1 + six and per_channel.min() > 0.1 - six, (per_channel.min(), per_channel.max())
