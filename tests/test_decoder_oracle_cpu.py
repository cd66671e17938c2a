"""oracle/decoder_ref.py pinned against the reference's own outputs: tests/golden/ococc_head.npz holds the logits the
imported reference's OccDecoder.occ_forward produced (oracle/gen_golden_ococc.py) for name-hashed weights."""
import os

import numpy as np
import pytest
import torch

from oracle import decoder_ref as D
from oracle import synth

PREFIX = 'occ_ae_head.occ_decoder.'
SHAPES = {'ln.weight': (1536,), 'ln.bias': (1536,),
          'conv_occ.0.0.weight': (512, 1596), 'conv_occ.0.1.weight': (512,), 'conv_occ.0.1.bias': (512,),
          'conv_occ.1.0.weight': (1024, 512), 'conv_occ.1.1.weight': (1024,), 'conv_occ.1.1.bias': (1024,),
          'conv_occ.2.0.weight': (1024, 1024), 'conv_occ.2.1.weight': (1024,), 'conv_occ.2.1.bias': (1024,),
          'conv_occ.3.weight': (1, 1024), 'conv_occ.3.bias': (1,)}


def decoder_params():
    return synth.synth_state_dict({PREFIX + k: s for k, s in SHAPES.items()}, seed=0)


def test_decoder_oracle_vs_reference_golden(golden_dir):
    gold = np.load(os.path.join(golden_dir, 'ococc_head.npz'))
    P = decoder_params()
    feats = torch.from_numpy(gold['out_fused_roi_feats'])
    xyz = torch.from_numpy(gold['dec_xyz'])
    R, K, _ = xyz.shape
    idx = torch.arange(R).repeat_interleave(K)
    logits = D.decoder(P, PREFIX, feats, xyz.reshape(-1, 3), idx).view(R, K, 1).numpy()
    ref = gold['dec_logits']
    assert np.abs(logits - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())
    # the bf16 roundings of the fused kernels move the logits by bf16-sized amounts, not more
    lo = D.decoder(P, PREFIX, feats, xyz.reshape(-1, 3), idx, rounding='bf16').view(R, K, 1).numpy()
    assert 1e-5 < np.abs(lo - ref).max() < 3e-2 * max(1.0, np.abs(ref).max())


def test_pos_encode_oracle_vs_reference_golden(golden_dir):
    gold = np.load(os.path.join(golden_dir, 'ococc_head.npz'))
    pe = D.pos_encode(torch.from_numpy(gold['posenc_in']).reshape(-1, 3)).numpy()
    assert np.allclose(pe.reshape(gold['posenc_out'].shape), gold['posenc_out'], atol=1e-6)


def _train_case(k, n, rows=200, seed=3):
    g = torch.Generator().manual_seed(seed + k + n)
    x = torch.randn(rows, k, generator=g).to(torch.bfloat16)
    W = torch.randn(n, k, generator=g) / k ** 0.5
    gam, bet = 1 + 0.2 * torch.randn(n, generator=g), 0.2 * torch.randn(n, generator=g)
    add = torch.randn(7, n, generator=g)
    idx = torch.randint(0, 7, (rows,), generator=g).sort().values
    hw, hb = torch.randn(n, generator=g) / 32, torch.tensor([-0.1])
    keep = torch.rand(rows, n, generator=g) >= 0.1
    return dict(x=x, W=W, ln_w=gam, ln_b=bet, eps=1e-3, add=add, idx=idx, head_w=hw, head_b=hb), keep


def test_train_rounding_is_bf16_rounding_with_z_rounded_first():
    """rounding='train' without a mask against rounding='bf16': the only difference is the rounding of z in front of
    the LayerNorm -- half a bf16 step, |dz_i| <= e_i = 2^-8 |z_i| (8 significant bits), per element.  To first order it moves the LayerNorm
    output h_i = (z_i - mu) rstd g_i + b_i by at most
        dh_i = rstd |g_i| (e_i + mean(e)) + |z_i - mu| rstd^3 |g_i| (1 / N) sum_j |z_j - mu| (e_j + mean(e))
    (the element itself, the shift of the mean, the shift of the variance), GELU' lies in [-0.13, 1.13], and the two
    roundings of y add half a step each: 2^-8 (|y_train| + |y_bf16|).  1 % on top for the second order."""
    for k, n in ((64, 512), (512, 1024), (1024, 1024)):
        kw, _ = _train_case(k, n)
        yb, hb = D.mlp_layer(rounding='bf16', **kw)
        yt, ht, z, mean, rstd = D.mlp_layer(rounding='train', **kw)
        assert torch.equal(z, D.r16(z)) and torch.equal(yt, D.r16(yt))   # both hold bf16 values
        zu = D.r16(kw['x']) @ D.r16(kw['W']).t() + kw['add'].double()[kw['idx']]
        assert torch.equal(z, D.r16(zu))
        e = 2.0 ** -8 * zu.abs()
        eb = e + e.mean(-1, keepdim=True)
        d = (zu - zu.mean(-1, keepdim=True)).abs()
        r = rstd.unsqueeze(-1)
        ga = kw['ln_w'].double().abs()
        dh = r * ga * eb + d * r ** 3 * ga * (d * eb).mean(-1, keepdim=True)
        tol = 1.01 * (1.13 * dh + 2.0 ** -8 * (yt.abs() + yb.abs()))
        diff = (yt - yb).abs()
        print(f'train vs bf16 {k}->{n}: largest difference / bound {float((diff / tol).max()):.3f}, '
              f'norm-wise {float(diff.norm() / yb.norm()):.2e}, equal {float((diff == 0).double().mean()):.3f}')
        assert bool((diff <= tol).all()), float((diff / tol).max())
        assert 0 < float(diff.norm() / yb.norm()) < 2.0 ** -8   # (they do differ, by less than a bf16 step norm-wise)
        # the head reads the rounded activation in both modes
        assert torch.equal(ht, yt @ kw['head_w'].double() + kw['head_b'].double().view(()))
        assert float((ht - hb).abs().max()) <= float(((yt - yb).abs() @ kw['head_w'].double().abs()).max()) + 1e-12


def test_train_rounding_statistics_are_those_of_the_returned_z():
    for k, n in ((64, 512), (1024, 1024)):
        kw, keep = _train_case(k, n)
        for kp in (None, keep):
            y, _, z, mean, rstd = D.mlp_layer(rounding='train', keep=kp, drop_threshold=6554 if kp is not None else 0, **kw)
            m = z.mean(-1)
            var = ((z - m.unsqueeze(-1)) ** 2).mean(-1)
            assert torch.allclose(mean, m, rtol=0, atol=1e-15) and torch.allclose(rstd, (var + 1e-3) ** -0.5, rtol=1e-14, atol=0)
            # ... and not those of the unrounded sums: the rounding moves the mean by far more than float64 does
            zu = D.r16(kw['x']) @ D.r16(kw['W']).t() + kw['add'].double()[kw['idx']]
            assert float((zu.mean(-1) - mean).abs().max()) > 1e-7
            # y is the activation of exactly these statistics
            h = (z - mean.unsqueeze(-1)) * rstd.unsqueeze(-1) * kw['ln_w'].double() + kw['ln_b'].double()
            a = D.gelu(h)
            if kp is not None:
                a = a * kp.double() * (65536.0 / (65536.0 - 6554))
            assert torch.equal(y, D.r16(a))


def test_train_rounding_keep_mask_drops_and_scales():
    kw, keep = _train_case(512, 1024)
    thr = 6554
    scale = 65536.0 / (65536.0 - thr)
    y0, h0, z0, _, _ = D.mlp_layer(rounding='train', **kw)
    y, h, z, _, _ = D.mlp_layer(rounding='train', keep=keep, drop_threshold=thr, **kw)
    assert torch.equal(z, z0)                                   # the mask sits behind the LayerNorm
    assert bool((y[~keep] == 0).all()) and bool((y0 != 0).all())   # (no activation of this input rounds to zero)
    # kept elements: scaled in front of the ONE rounding -- within half a step of scale * (the rounded undropped value's
    # pre-image), i.e. |y - scale y0| <= 2^-8 |y| + scale 2^-8 |y0|
    kept = (y - scale * y0).abs()[keep]
    assert bool((kept <= 2.0 ** -8 * (y.abs() + scale * y0.abs())[keep]).all())
    assert float((y[keep] / y0[keep]).mean()) == pytest.approx(scale, rel=1e-3)
    assert torch.equal(h, y @ kw['head_w'].double() + kw['head_b'].double().view(()))   # the head reads the dropped activation
    with pytest.raises(AssertionError):
        D.mlp_layer(rounding='bf16', keep=keep, **kw)


def test_train_rounding_is_straight_through_for_autograd():
    """the roundings pass gradients unchanged: d head / d z-path equals that of the same forward without roundings up to
    the roundings' effect on the VALUES (no gradient is cast to bf16 on the way back)."""
    kw, keep = _train_case(64, 512, rows=33)
    W = kw.pop('W').double().requires_grad_(True)
    add = kw.pop('add').double().requires_grad_(True)
    y, h, _, _, _ = D.mlp_layer(W=W, add=add, rounding='train', keep=keep, drop_threshold=6554, **kw)
    h.sum().backward()
    gW, gadd = W.grad.clone(), add.grad.clone()
    assert gW.dtype == torch.float64 and not torch.equal(gW, D.r16(gW))   # float64 values, not bf16 ones
    W2, add2 = W.detach().clone().requires_grad_(True), add.detach().clone().requires_grad_(True)
    z = kw['x'].double() @ W2.t() + add2[kw['idx']]
    a = D.gelu(D.layer_norm(z, kw['ln_w'], kw['ln_b'], 1e-3)) * keep.double() * (65536.0 / (65536.0 - 6554))
    (a @ kw['head_w'].double() - 0.1).sum().backward()
    assert float((gW - W2.grad).norm() / W2.grad.norm()) < 2e-2 and float((gadd - add2.grad).norm() / add2.grad.norm()) < 2e-2
