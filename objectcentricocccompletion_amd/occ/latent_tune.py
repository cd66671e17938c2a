"""Test-time tuning of the RoI latents on kernels (csrc/latent_tune.hip) -- the MI355X form of
OccAutoEncoder.online_tuning_forward (occ_ae_head.py:346-391) for the bf16 decoder: ``num_iter`` Adam steps on the
observation loss of the frozen decoder, without autograd.  Per iteration, all on the current stream, no read-back:

    n        = LN(e)                                   ococc_layernorm_act_fwd (f32, act none; skipped without use_ln)
    roi_part = n W_roi^T                               library GEMM, [K, 512]
    logits   = decoder(pe, roi_part[idx])              ococc_occ_mlp_train_fwd_bf16 (threshold 0), leaves z / stats / y
    dz2      = loss', head', LN+GELU' of layer 2       ococc_occ_tune_head_lnbwd_bf16      (kernel A)
    dy1 = dz2 W2,  dz1 = LN+GELU' of layer 1           library GEMM, ococc_layernorm_act_bwd (null dgamma / dbeta)
    dy0 = dz1 W1,  dz0 = LN+GELU' of layer 0                 "
    d_roi    = segment sum of dz0 over idx             ococc_segment_sum_bf16              (kernel B), f32 [K, 512]
    d_n      = d_roi W_roi                             library GEMM, [K, D]
    e, m, v  = Adam(e, LN'(d_n))                       ococc_latent_ln_adam_f32            (kernel C)

Every buffer is allocated once per call: z, y and stats of the three layers (10.3 KB per sampled row), the gradient
buffers (6.1 KB per row), the bf16 copies of W1 and W2, the positional encoding and the operand fragments."""
import ctypes
import os

import torch

from .. import _lib as L
from . import fused_mlp as fm

# 0: OccBBoxHead.online_tuning takes OccAutoEncoder.online_tuning_forward (autograd) whatever the decoder
KERNELS = os.environ.get('OCOCC_LATENT_TUNE_KERNELS', '1') != '0'

ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8   # torch.optim.Adam's defaults, as the reference constructs it


def decoder_layers(decoder):
    """(layers, head) of ``decoder`` when tune_latents takes it -- the bf16 decoder of the shape _forward_fused_train
    accepts (60 -> 512 -> 1024 -> 1024 -> 1, LayerNorm + GELU, no Linear bias) -- else None."""
    if getattr(decoder, 'compute_dtype', None) != torch.bfloat16 or not isinstance(decoder.conv_occ, torch.nn.Sequential):
        return None
    fused = decoder._fused_layers()
    if fused is None:
        return None
    layers, head = fused
    D = decoder.roi_feature_channels
    lin0 = layers[0][0]
    widths = (fm.pad64(lin0.in_features - D),) + tuple(l.out_features for l, _ in layers)
    if not (len(layers) == 3 and widths == fm.OCC_MLP_WIDTHS and all(l.bias is None for l, _ in layers)
            and len({ln.eps for _, ln in layers}) == 1 and head.bias is not None
            and all(p.dtype == torch.float32 for l, ln in layers for p in (l.weight, ln.weight, ln.bias))
            and 4 <= D <= 2048 and D % 4 == 0):
        return None
    return layers, head


def supported(decoder, *tensors):
    return KERNELS and all(t is None or t.is_cuda for t in tensors) and decoder_layers(decoder) is not None


def _ln_bwd(z, dy, g, b, stats, dz, ws):
    n, c = z.shape
    L.check(L.lib.ococc_layernorm_act_bwd(L.ptr(z), L.ptr(dy), n, c, L.ptr(g), L.ptr(b), L.ptr(stats), 1, L.ptr(dz), None,
                                          None, L.BF16, L.ptr(ws), ws.numel(), L.stream()), 'latent_tune: layernorm_act_bwd')


@torch.no_grad()
def tune_latents(decoder, latents, smp_xyz, labels, roi_index, num_iter, weights=None, lr=0.01, step_size=1000, gamma=0.1,
                 loss_weight=1.0, debug=False):
    """latents f32 [K, D], smp_xyz f32 [M, 3], labels [M] (0 / 1), roi_index [M] non-decreasing in [0, K), weights [M]
    or None -> the tuned latents (a new tensor) after ``num_iter`` steps of Adam(lr) under StepLR(step_size, gamma) on
    mean(loss_weight * weights * BCE(decoder(latents)[i], labels[i])).  ``debug``: (tuned, dict(de = the latent gradient
    of the first iteration, logits = the logits of the first iteration))."""
    spec = decoder_layers(decoder)
    if spec is None:
        raise L.OcoccError('tune_latents: the decoder is outside the tuning kernels (bf16 compute_dtype, 60 -> 512 -> '
                           '1024 -> 1024 -> 1 with LayerNorm + GELU and no Linear bias)')
    L.require_device(latents, smp_xyz, labels, roi_index, weights)
    layers, head = spec
    dev, bf, f32 = latents.device, torch.bfloat16, torch.float32
    e = latents.detach().to(f32).clone().contiguous()
    K, D = e.shape
    M = smp_xyz.size(0)
    info = {}
    if M == 0 or K == 0 or num_iter <= 0:
        return (e, info) if debug else e
    lin0 = layers[0][0]
    w_roi = lin0.weight.detach()[:, :D]                                     # [512, D] view
    c32 = lambda t: t.detach().to(f32).contiguous()
    gs, bs = [c32(ln.weight) for _, ln in layers], [c32(ln.bias) for _, ln in layers]
    hw, hb = c32(head.weight).view(-1), c32(head.bias).view(-1)
    eps = float(layers[0][1].eps)
    w1b, w2b = layers[1][0].weight.detach().to(bf), layers[2][0].weight.detach().to(bf)
    if not hasattr(decoder, '_train_weights'):
        decoder._train_weights = fm.DecoderWeights()
    frags = decoder._train_weights.get([lin0.weight[:, D:], layers[1][0].weight, layers[2][0].weight],
                                       [fm.pad64(lin0.in_features - D), layers[1][0].in_features, layers[2][0].in_features])
    bound = decoder.pos_encode.norm_bound if decoder.pos_encode.use_norm else None
    pe = fm.pos_encode_bf16(smp_xyz, decoder.pos_encode.L, bound)
    idx = roi_index.to(torch.int32).contiguous()
    lab = labels.to(torch.int32).contiguous()
    wts = None if weights is None else c32(weights)
    use_ln = bool(decoder.use_ln)
    ln_g = c32(decoder.ln.weight) if use_ln else None
    ln_b = c32(decoder.ln.bias) if use_ln else None
    ln_eps = float(decoder.ln.eps) if use_ln else 0.0

    widths = fm.OCC_MLP_WIDTHS[1:]
    zs = [torch.empty((M, n), dtype=bf, device=dev) for n in widths]
    ys = [torch.empty((M, n), dtype=bf, device=dev) for n in widths]
    stats = [torch.empty((M, 2), dtype=f32, device=dev) for _ in widths]
    logits = torch.empty((M,), dtype=f32, device=dev)
    dz2, dy1 = torch.empty_like(zs[2]), torch.empty_like(zs[1])
    dz1 = dz2   # (dz2 is dead once dy1 = dz2 W2 is taken; the LayerNorm backward never reads and writes one buffer)
    dy0, dz0 = torch.empty_like(zs[0]), torch.empty_like(zs[0])
    n_buf = torch.empty_like(e) if use_ln else None
    n_stats = torch.empty((K, 2), dtype=f32, device=dev) if use_ln else None
    roi_part = torch.empty((K, widths[0]), dtype=f32, device=dev)
    d_roi = torch.empty((K, widths[0]), dtype=f32, device=dev)
    d_n = torch.empty((K, D), dtype=f32, device=dev)
    m, v = torch.zeros_like(e), torch.zeros_like(e)
    de = torch.empty_like(e) if debug else None
    ws = L.workspace(max(L.lib.ococc_layernorm_act_bwd_workspace_bytes(M, widths[1]),
                         L.lib.ococc_layernorm_act_bwd_workspace_bytes(M, widths[0])), dev)
    vp = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    p_frag, p_g, p_b, p_z, p_y, p_s = vp(frags), vp(gs), vp(bs), vp(zs), vp(ys), vp(stats)
    scale = float(loss_weight) / M
    w_roi_t = w_roi.t()
    for it in range(num_iter):
        if use_ln:
            L.check(L.lib.ococc_layernorm_act_fwd(L.ptr(e), K, D, L.ptr(ln_g), L.ptr(ln_b), ln_eps, 0, L.ptr(n_buf),
                                                  L.ptr(n_stats), L.F32, L.stream()), 'latent_tune: layernorm_act_fwd')
        torch.mm(n_buf if use_ln else e, w_roi_t, out=roi_part)
        L.check(L.lib.ococc_occ_mlp_train_fwd_bf16(
            L.ptr(pe), M, L.ptr(roi_part), L.ptr(idx), p_frag, p_g, p_b, eps, L.ptr(hw), L.ptr(hb), 0, None, p_z, p_y, p_s,
            L.ptr(logits), L.stream()), 'latent_tune: occ_mlp_train_fwd')
        if debug and it == 0:
            info['logits'] = logits.clone()
        L.check(L.lib.ococc_occ_tune_head_lnbwd_bf16(
            L.ptr(logits), L.ptr(lab), L.ptr(wts), scale, L.ptr(hw), L.ptr(zs[2]), L.ptr(stats[2]), L.ptr(gs[2]),
            L.ptr(bs[2]), M, widths[2], L.ptr(dz2), L.stream()), 'latent_tune: occ_tune_head_lnbwd')
        torch.mm(dz2, w2b, out=dy1)
        _ln_bwd(zs[1], dy1, gs[1], bs[1], stats[1], dz1, ws)
        torch.mm(dz1, w1b, out=dy0)
        _ln_bwd(zs[0], dy0, gs[0], bs[0], stats[0], dz0, ws)
        L.check(L.lib.ococc_segment_sum_bf16(L.ptr(dz0), L.ptr(idx), M, widths[0], L.ptr(d_roi), K, L.stream()),
                'latent_tune: segment_sum')
        torch.mm(d_roi, w_roi, out=d_n)
        L.check(L.lib.ococc_latent_ln_adam_f32(
            L.ptr(e), L.ptr(d_n), L.ptr(m), L.ptr(v), K, D, L.ptr(ln_g), ln_eps, int(use_ln),
            float(lr) * float(gamma) ** (it // int(step_size)), ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS, it + 1,
            L.ptr(de) if (debug and it == 0) else None, L.stream()), 'latent_tune: latent_ln_adam')
    if debug:
        info['de'] = de
        return e, info
    return e
