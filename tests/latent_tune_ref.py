"""Plain float64 restatement of the latent-tuning kernels (csrc/latent_tune.hip) and of one whole tuning iteration
(occ/latent_tune.py), written out from the formulas without autograd: the tests compare the kernels with this file, and
this file with torch's float64 autograd + torch.optim.Adam / StepLR (tests/test_latent_tune_cpu.py).  The tensor functions
run on whatever device their inputs are on."""
import math

import torch

import ln_ref
from oracle import decoder_ref as D

F64 = torch.float64


def _f64(t, like=None):
    t = torch.as_tensor(t)
    return t.to(device=t.device if like is None else like.device, dtype=F64)


def loss_grad(logits, labels, weights, scale):
    """d [M] = scale * w_i * (sigmoid(logit_i) - label_i): the gradient of mean(loss_weight * w * BCE-with-logits) with
    scale = loss_weight / M.  sigmoid - label through the numerically exact branch for each sign of the logit."""
    x = _f64(logits)
    y = _f64(labels, x)
    en = torch.exp(-x.abs())
    # label 1: sigmoid - 1 = -1 / (1 + e^x);  label 0: sigmoid = 1 / (1 + e^-x); both without cancellation
    pos = torch.where(x >= 0, 1.0 / (1.0 + en), en / (1.0 + en))       # sigmoid(x)
    neg = torch.where(x >= 0, en / (1.0 + en), 1.0 / (1.0 + en))       # 1 - sigmoid(x)
    diff = torch.where(y > 0.5, -neg, pos)
    w = torch.ones_like(x) if weights is None else _f64(weights, x)
    return float(scale) * w * diff


def head_lnbwd(logits, labels, weights, scale, head_w, z, mean, rstd, gamma, beta):
    """Kernel A.  -> dict(dz [M, C], d [M], unit [M, C]): dz = LayerNorm+GELU backward (ln_ref, from the STORED mean /
    rstd) of dy = d * head_w; ``unit`` = rstd (a_c + mean_c a + |xhat_c| mean_c (a |xhat|)) with a_c = |head_w_c gamma_c|:
    the magnitude per unit of |d| that an error bound of dz scales with (|GELU'| <= 1.13 is left out of a_c)."""
    d = loss_grad(logits, labels, weights, scale)
    hw = _f64(head_w, d).view(1, -1)
    dy = d[:, None] * hw
    t = ln_ref.ln_act_backward_terms(z, dy, gamma, beta, 0.0, 1, stats=(mean, rstd))
    a = (hw * _f64(gamma, d).view(1, -1)).abs().expand_as(t['xhat'])
    ax = t['xhat'].abs()
    unit = t['rstd'][:, None] * (a + a.mean(1, keepdim=True) + ax * (a * ax).mean(1, keepdim=True))
    return dict(dz=t['dx'], d=d, unit=unit)


def segment_sum(x, index, num_segments):
    """Kernel B.  -> (sum [K, C], sum of |x| [K, C], rows per segment [K]) of the rows of x whose index is k."""
    x = _f64(x)
    idx = torch.as_tensor(index).to(x.device).long()
    ok = (idx >= 0) & (idx < num_segments)
    out = torch.zeros((num_segments, x.shape[1]), dtype=F64, device=x.device)
    out_abs = torch.zeros_like(out)
    out.index_add_(0, idx[ok], x[ok])
    out_abs.index_add_(0, idx[ok], x[ok].abs())
    return out, out_abs, torch.bincount(idx[ok], minlength=num_segments)


def ln_backward_input(e, d_n, gamma, ln_eps):
    """de of n = LN(e) * gamma + beta given d_n (plain LayerNorm: ln_ref with act none)."""
    return ln_ref.ln_act_backward_terms(e, d_n, gamma, torch.zeros_like(_f64(gamma)), ln_eps, 0)['dx']


def latent_ln_adam(e, d_n, m, v, gamma, ln_eps, use_ln, lr, beta1, beta2, eps, t):
    """Kernel C.  -> (e', m', v', de): torch.optim.Adam's step t (from 1) with the step's learning rate lr."""
    e, d_n, m, v = _f64(e), _f64(d_n), _f64(m), _f64(v)
    de = ln_backward_input(e, d_n, gamma, ln_eps) if use_ln else d_n
    m1 = m + (de - m) * (1.0 - beta1)
    v1 = beta2 * v + (1.0 - beta2) * de * de
    denom = torch.sqrt(v1) / math.sqrt(1.0 - beta2 ** t) + eps
    return e - (lr / (1.0 - beta1 ** t)) * (m1 / denom), m1, v1, de


def step_lr(lr, step_size, gamma, it):
    """learning rate of iteration ``it`` (from 0) under StepLR"""
    return lr * gamma ** (it // step_size)


def decoder_forward(P, pe, n, idx, rounding=None):
    """The decoder's three hidden layers and head on n [K, D] (the latent behind its LayerNorm), pe [M, 60], idx [M].
    P: dict(W_roi [512, D], W_pe [512, 60], W1, W2, g = [3], b = [3], hw [1024], hb [1], eps).  rounding None or 'train'
    (oracle/decoder_ref.py).  -> dict(logits [M], z, mean, rstd: per layer, W: the operand weights)."""
    rd = D.r16 if rounding == 'train' else _f64
    roi_part = n @ _f64(P['W_roi']).t()
    if rounding == 'train':
        roi_part = roi_part.to(torch.float32).to(F64)
    Ws = [rd(P['W_pe']), rd(P['W1']), rd(P['W2'])]
    x = rd(pe)
    out = dict(z=[], mean=[], rstd=[], W=Ws)
    for l in range(3):
        z = x @ Ws[l].t()
        if l == 0:
            z = z + roi_part[idx.long()]
        if rounding == 'train':
            z = D.r16(z)
        y, mean, rstd = ln_ref.ln_act(z, P['g'][l], P['b'][l], P['eps'], 1)
        out['z'].append(z), out['mean'].append(mean), out['rstd'].append(rstd)
        x = rd(y)
    out['logits'] = x @ _f64(P['hw']).view(-1) + _f64(P['hb']).view(())
    return out


def latent_gradient(P, pe, e, idx, labels, weights, loss_weight, rounding=None):
    """de [K, D] of mean(loss_weight * w * BCE(decoder(e))) by hand, every rounding straight-through, and the logits."""
    e = _f64(e)
    K = e.shape[0]
    if P['use_ln']:
        n = ln_ref.ln_act(e, P['ln_g'], P['ln_b'], P['ln_eps'], 0)[0]
    else:
        n = e
    f = decoder_forward(P, pe, n, idx, rounding)
    M = pe.shape[0]
    dz = head_lnbwd(f['logits'], labels, weights, loss_weight / M, P['hw'], f['z'][2], f['mean'][2], f['rstd'][2],
                    P['g'][2], P['b'][2])['dz']
    for l in (1, 0):
        dy = dz @ f['W'][l + 1]
        dz = ln_ref.ln_act_backward_terms(f['z'][l], dy, P['g'][l], P['b'][l], 0.0, 1, stats=(f['mean'][l], f['rstd'][l]))['dx']
    d_roi = segment_sum(dz, idx, K)[0]
    d_n = d_roi @ _f64(P['W_roi'])
    de = ln_backward_input(e, d_n, P['ln_g'], P['ln_eps']) if P['use_ln'] else d_n
    return de, d_n, f['logits']


def tune(P, pe, e, idx, labels, weights, num_iter, lr=0.01, step_size=1000, gamma=0.1, betas=(0.9, 0.999), eps=1e-8,
         loss_weight=1.0, rounding=None):
    """``num_iter`` whole iterations -> (e, [de of every iteration])."""
    e = _f64(e).clone()
    m, v = torch.zeros_like(e), torch.zeros_like(e)
    des = []
    for it in range(num_iter):
        _, d_n, _ = latent_gradient(P, pe, e, idx, labels, weights, loss_weight, rounding)
        e, m, v, de = latent_ln_adam(e, d_n, m, v, P.get('ln_g'), P.get('ln_eps', 0.0), P['use_ln'],
                                     step_lr(lr, step_size, gamma, it), betas[0], betas[1], eps, it + 1)
        des.append(de)
    return e, des
