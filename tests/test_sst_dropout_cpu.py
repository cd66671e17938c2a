"""Attention dropout of the SST blocks (csrc/attn_dropout.hpp), host side: the reference's default dropout=0.1 builds
(sst_basic_block_v2.py:79-81, 133), with the parameter layout of the dropout-free modules, and the restated keep mask
has the distribution it promises.  The restatement (``keep``) is the one tests/test_gpu_sst_dropout.py holds the
kernels to, bit for bit."""
import numpy as np
import pytest
import torch

M32 = np.uint32(0xFFFFFFFF)


def _fmix(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def _fold(state, word):
    return _fmix((state ^ word) * np.uint32(0x9E3779B1) + np.uint32(0x7F4A7C15))


def keep(seed, head, q_row, k_row, p):
    """keep(seed64, head, q, k) = hash24(seed, head, q, k) >= floor(p * 2^24), numpy uint32 arithmetic (wraps mod 2^32)"""
    with np.errstate(over='ignore'):
        seed = int(seed)
        s = _fold(_fmix(np.uint32(seed & 0xFFFFFFFF) ^ np.uint32(0x3C6EF372)), np.uint32(seed >> 32))
        st = _fold(s, np.asarray(head, dtype=np.int64).astype(np.uint32))
        h = _fold(_fold(st, np.asarray(k_row, dtype=np.int64).astype(np.uint32)),
                  np.asarray(q_row, dtype=np.int64).astype(np.uint32))
    thr = np.uint32(int(float(np.float32(p)) * 16777216.0))
    return (h >> np.uint32(8)) >= thr


def _sst(dropout, cosine):
    from objectcentricocccompletion_amd.sst.sst_modules import SSTv2
    return SSTv2(d_model=[128] * 2, nhead=[8] * 2, num_blocks=2, dim_feedforward=[256] * 2, dropout=dropout,
                 activation='gelu', layer_cfg=dict(cosine=True) if cosine else dict())


def _layout(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_reference_default_dropout_constructs_with_the_same_parameters():
    from objectcentricocccompletion_amd.sst.sst_modules import BasicShiftBlockV2, EncoderLayer
    enc = EncoderLayer(128, 8, 256)                       # dropout=0.1, the reference's default
    assert enc.win_attn.self_attn.dropout == pytest.approx(0.1)
    assert _layout(enc) == _layout(EncoderLayer(128, 8, 256, dropout=0.0))
    blk = BasicShiftBlockV2(128, 8, 256)
    assert _layout(blk) == _layout(BasicShiftBlockV2(128, 8, 256, dropout=0.0))
    for cosine in (False, True):
        assert _layout(_sst(0.1, cosine)) == _layout(_sst(0.0, cosine))


@pytest.mark.parametrize('bad', [-0.1, 1.0, 1.5])
def test_dropout_outside_zero_one_is_refused(bad):
    from objectcentricocccompletion_amd.sst.sst_modules import EncoderLayer
    with pytest.raises(ValueError):
        EncoderLayer(128, 8, 256, dropout=bad)


def test_encoder_layer_keeps_attention_dropout_on_the_fused_kernels():
    """attention dropout alone stays on the tile kernels; mlp_dropout in training mode still falls back"""
    from objectcentricocccompletion_amd.sst.sst_modules import EncoderLayer
    enc = EncoderLayer(128, 8, 256, 0.1, 'gelu', layer_cfg=dict(compute_dtype=torch.bfloat16)).train()
    assert enc._fusable()
    enc2 = EncoderLayer(128, 8, 256, 0.1, 'gelu', mlp_dropout=0.1, layer_cfg=dict(compute_dtype=torch.bfloat16)).train()
    assert not enc2._fusable()
    assert enc2.eval()._fusable()


def test_eval_and_zero_dropout_draw_no_seed():
    from objectcentricocccompletion_amd.sst.sst_modules import WindowMultiheadAttention
    m = WindowMultiheadAttention(128, 8, dropout=0.1)
    assert m.eval().drop_args(torch.device('cpu')) == (0.0, None)
    assert WindowMultiheadAttention(128, 8, dropout=0.0).train().drop_args(torch.device('cpu')) == (0.0, None)
    p, seed = m.train().drop_args(torch.device('cpu'))
    assert p == pytest.approx(0.1) and seed.dtype == torch.int64 and seed.shape == (1,)


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_restated_mask_statistics(p):
    """over >= 10^6 pairs (rows in the millions, as at configs[4] sizes) the dropped fraction is p within 5 sigma; under
    two seeds, and for (q, k) against (k, q), the jointly dropped fraction is p^2 within 5 sigma"""
    rng = np.random.default_rng(0)
    n = 1 << 21
    q = rng.integers(0, 5_000_000, n)
    k = rng.integers(0, 5_000_000, n)
    h = rng.integers(0, 8, n)
    s1, s2 = 0x1234_5678_9ABC_DEF0 >> 2, 987654321012345
    d1 = ~keep(s1, h, q, k, p)
    sig = np.sqrt(p * (1 - p) / n)
    assert abs(d1.mean() - p) < 5 * sig, (d1.mean(), p)
    d2 = ~keep(s2, h, q, k, p)
    dt = ~keep(s1, h, k, q, p)
    sig2 = np.sqrt(p * p * (1 - p * p) / n)
    for both in (d1 & d2, d1 & dt):
        assert abs(both.mean() - p * p) < 5 * sig2, (both.mean(), p * p)
    # consecutive rows of one window (the pairs one query sees) are no more alike than random pairs
    qq = np.repeat(np.arange(n // 16), 16)
    kk = np.tile(np.arange(16), n // 16) + 3_000_000
    d = ~keep(s1, 0, qq, kk, p)
    assert abs(d.mean() - p) < 5 * sig
    assert abs((d[1:] & d[:-1]).mean() - p * p) < 5 * sig2
