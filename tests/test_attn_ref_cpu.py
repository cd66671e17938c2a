"""tests/attn_ref.py checked on its own, on the CPU: the float64 chain against torch's scaled_dot_product_attention, and
the numpy restatement of the dropout hash (attn_keep of csrc/causal_attn.hip) as a random number generator -- the GPU
tests compare the kernel's mask with it bit for bit, so what is checked here is that the hash they pin down is a usable
one: the right share dropped overall and per (tracklet, head), no dependence between heads, between neighbours along a
row or between seeds, and both halves of the 64-bit seed taking part."""
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R        # noqa: E402

SEEDS = (0, 1, 123456789, 123456790, 123456789 + 2 ** 32, 2 ** 32, 2 ** 62 - 1)
SHAPES = ((4, 200, 200), (6, 70, 130), (2, 256, 256))
SIGMAS = 5.0


def test_float64_chain_is_scaled_dot_product_attention():
    B, H, L, S, D = 3, 2, 37, 53, 20
    g = torch.Generator().manual_seed(11)
    q = torch.randn(L * B, H * D, generator=g, dtype=torch.float64)
    k = torch.randn(S * B, H * D, generator=g, dtype=torch.float64)
    v = torch.randn(S * B, H * D, generator=g, dtype=torch.float64)
    attn_mask = torch.triu(torch.ones(L, S, dtype=torch.bool), 1 + S - L)
    lens = torch.tensor([S, 1, 30])
    key_pad = torch.arange(S)[None, :] >= lens[:, None]
    got = R.attention(q, k, v, (B, H, L, S, D), attn_mask, key_pad)
    bhnd = lambda t, n: t.reshape(n, B, H, D).permute(1, 2, 0, 3)
    allowed = ~R.combined_mask(B, H, L, S, attn_mask, key_pad)
    assert bool(allowed.any(-1).all()) and not bool(allowed.all())
    ref = torch.nn.functional.scaled_dot_product_attention(bhnd(q, L), bhnd(k, S), bhnd(v, S), attn_mask=allowed)
    ref = ref.permute(2, 0, 1, 3).reshape(L * B, H * D)
    assert float((got - ref).abs().max()) <= 1e-12
    # the two masks one at a time, and none
    for am, kp in ((attn_mask, None), (None, key_pad), (None, None)):
        m = R.combined_mask(B, H, L, S, am, kp)
        ref = torch.nn.functional.scaled_dot_product_attention(bhnd(q, L), bhnd(k, S), bhnd(v, S),
                                                               attn_mask=None if m is None else ~m)
        got = R.attention(q, k, v, (B, H, L, S, D), am, kp)
        assert float((got - ref.permute(2, 0, 1, 3).reshape(L * B, H * D)).abs().max()) <= 1e-12


def test_keep_and_scale_of_the_chain():
    """keep multiplies the probabilities behind the softmax, scaled by 1 / (1 - p)"""
    B, H, L, S, D = 1, 2, 5, 7, 4
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(n * B, H * D, generator=g, dtype=torch.float64) for n in (L, S, S))
    keep = torch.rand(B * H, L, S, generator=g) < 0.5
    prob = R.probabilities(q, k, (B, H, L, S, D), None, None)
    want = torch.bmm(prob * keep * 2.0, R.heads(v, S, B, H, D)).transpose(0, 1).reshape(L * B, H * D)
    assert torch.equal(R.attention(q, k, v, (B, H, L, S, D), None, None, keep=keep.numpy(), p=0.5), want)


def _z(count, n, expect):
    return (count / n - expect) / math.sqrt(expect * (1.0 - expect) / n)


@pytest.mark.parametrize('p', [0.01, 0.1, 0.5])
@pytest.mark.parametrize('BH,L,S', SHAPES)
def test_dropout_hash_statistics(BH, L, S, p):
    """every share within 5 standard deviations of its binomial expectation"""
    drop = {seed: ~R.keep_mask(seed, BH, L, S, p) for seed in SEEDS}
    worst = 0.0

    def check(what, count, n, expect):
        nonlocal worst
        z = _z(float(count), n, expect)
        worst = max(worst, abs(z))
        assert abs(z) <= SIGMAS, f'{what}: {count} of {n}, expected share {expect}: {z:+.2f} sigma'

    same = p * p + (1.0 - p) * (1.0 - p)
    for seed, d in drop.items():
        check(f'seed {seed}: dropped', d.sum(), d.size, p)
        for bh in range(BH):
            check(f'seed {seed}: dropped in bh {bh}', d[bh].sum(), L * S, p)
        check(f'seed {seed}: bh 0 and bh 1 agree', (d[0] == d[1]).sum(), L * S, same)
        check(f'seed {seed}: both dropped at lag 1 along s', (d[:, :, 1:] & d[:, :, :-1]).sum(), BH * L * (S - 1), p * p)
    for a, b in itertools.combinations(SEEDS, 2):
        check(f'seeds {a} and {b} agree', (drop[a] == drop[b]).sum(), drop[a].size, same)
    print(f'ATTNHASH BH={BH} L={L} S={S} p={p}: worst |z| {worst:.2f}')


def test_both_seed_words_take_part():
    BH, L, S, p = 2, 32, 32, 0.1
    m = lambda seed: R.keep_mask(seed, BH, L, S, p)
    assert not np.array_equal(m(123456789), m(123456789 + 2 ** 32))        # the high word alone
    assert not np.array_equal(m(0), m(2 ** 32))
    assert not np.array_equal(m(123456789), m(123456790))                  # the low word alone
    assert not np.array_equal(m(2 ** 32), m(123456789 + 2 ** 32))


def test_keep_mask_threshold_and_index():
    """thr = uint32(float32(p) * 2^24); p = 0 keeps everything; element (bh, l, s) has counter (bh L + l) S + s, so the
    mask of a larger BH starts with the mask of a smaller one"""
    assert int(R.drop_threshold(0.5)) == 2 ** 23 and int(R.drop_threshold(0.0)) == 0
    assert int(R.drop_threshold(0.1)) == int(np.float32(0.1) * np.float32(2 ** 24)) == 1677721
    assert R.keep_mask(7, 3, 5, 9, 0.0).all()
    big, small = R.keep_mask(99, 4, 6, 10, 0.3), R.keep_mask(99, 2, 6, 10, 0.3)
    assert big.shape == (4, 6, 10) and big.dtype == bool and np.array_equal(big[:2], small)
    # one element by hand, in Python integers
    seed, idx = 123456789 + (77 << 32), (1 * 6 + 4) * 10 + 3
    M = 0xffffffff
    h = (idx ^ (seed & M)) & M
    h = (h * 0x9E3779B1) & M
    h ^= h >> 16
    h = ((h + (seed >> 32)) * 0x85EBCA6B) & M
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M
    h ^= h >> 16
    assert bool(R.keep_mask(seed, 2, 6, 10, 0.3)[1, 4, 3]) == ((h >> 8) >= int(R.drop_threshold(0.3)))


def test_slice_error_is_per_tracklet_and_head():
    B, H, D, n = 2, 3, 4, 5
    ref = torch.ones(n * B, H * D, dtype=torch.float64)
    ref.view(n, B, H, D)[:, 1, 2] *= 1e-3             # a slice with small values
    ref.view(n, B, H, D)[:, 0, 1] = 0.0               # a zero slice
    got = ref.clone()
    got.view(n, B, H, D)[2, 1, 2, 3] += 1e-6          # 1e-3 of its slice, 1e-6 of the tensor
    got.view(n, B, H, D)[4, 0, 1, 0] = 0.25
    rel, zero_abs = R.slice_error(got, ref, B, H, D)
    assert abs(rel - 1e-3) <= 1e-12 and zero_abs == 0.25
    assert R.slice_error(ref, ref, B, H, D) == (0.0, 0.0)
    got.view(n, B, H, D)[0, 0, 0, 0] = float('nan')
    assert math.isnan(R.slice_error(got, ref, B, H, D)[0])
