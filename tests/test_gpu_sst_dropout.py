"""Attention dropout in the SST window-attention kernels (csrc/attn_dropout.hpp; the dropout_p / seed arguments of
ococc_window_attn_{fwd,bwd}_bf16 and ococc_window_attn_block_{fwd,bwd}_bf16): the mask is the specified hash bit for
bit, in the padded, gather and tile kernels alike; the kernels match a float64 restatement of the rounded chain with that
mask; the fused layer agrees with the operator path under the same seed; the statistics, eval mode and graph capture
behave as nn.MultiheadAttention's."""
import numpy as np
import pytest
import torch

from test_sst_dropout_cpu import keep
from test_gpu_sst_fused import DROP, SPARSE, WINDOW, _layer, _norm_err, _scene

pytestmark = pytest.mark.gpu

H, D, E = 8, 16, 128


def _r16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _seed(dev, value):
    return torch.tensor([value], dtype=torch.int64, device=dev)


def _windows(g, nW, T, dev, full=False):
    key_len = torch.full((nW,), T, dtype=torch.int32) if full else torch.randint(1, T + 1, (nW,), generator=g).int()
    return key_len.to(dev)


def _padded_mask(seed, key_len, T, p):
    """[nW, H, T(query), T(key)] keep mask of the padded entry points (rows w * T + t), False outside the windows"""
    nW = len(key_len)
    w, h, qi, ki = np.meshgrid(np.arange(nW), np.arange(H), np.arange(T), np.arange(T), indexing='ij')
    kl = key_len.cpu().numpy()[w]
    return keep(seed, h, w * T + qi, w * T + ki, p) & (qi < kl) & (ki < kl)


def _one_hot_v(nW, T, dev):
    """q = k = 0 (uniform probabilities), v of head h = e_{slot}: the output of head h is P_drop itself"""
    v = torch.zeros(nW, T, H, D)
    for t in range(T):
        v[:, t, :, t] = 1.0
    return v.reshape(nW, T, E).to(dev).bfloat16()


def test_padded_and_gather_masks_are_the_specified_hash(dev):
    from objectcentricocccompletion_amd import _lib as L
    g = torch.Generator().manual_seed(3)
    nW, T, p, sv = 23, 16, 0.3, 0x5EED_0001_2345
    key_len = _windows(g, nW, T, dev)
    q = torch.zeros(nW, T, E, dtype=torch.bfloat16, device=dev)
    v = _one_hot_v(nW, T, dev)
    out = torch.empty_like(q)
    lse = torch.empty((nW, H, T), dtype=torch.float32, device=dev)
    seed = _seed(dev, sv)
    L.check(L.lib.ococc_window_attn_fwd_bf16(L.ptr(q), L.ptr(q), L.ptr(v), E, E, E, None, L.ptr(key_len), nW, T, H, D,
                                             D ** -0.5, L.ptr(out), E, L.ptr(lse), p, L.ptr(seed), L.stream()), 'fwd')
    got = out.float().view(nW, T, H, D).permute(0, 2, 1, 3).cpu().numpy() != 0      # [nW, H, query, key slot]
    exp = _padded_mask(sv, key_len, T, p)
    live = np.arange(T)[None, None, :, None] < key_len.cpu().numpy()[:, None, None, None]
    assert np.array_equal(got & live, exp)
    # gather form, windows full and laid out in order: rows w * T + t coincide with the padded rows -> the same mask
    full = _windows(g, nW, T, dev, full=True)
    tok = torch.arange(nW * T, dtype=torch.int32, device=dev)
    qkv = torch.cat([q, q, v], 2).view(nW * T, 3 * E).contiguous()
    b = qkv.data_ptr()
    out_g = torch.empty((nW * T, E), dtype=torch.bfloat16, device=dev)
    L.check(L.lib.ococc_window_attn_fwd_bf16(b, b + 2 * E, b + 4 * E, 3 * E, 3 * E, 3 * E, L.ptr(tok),
                                             L.ptr(full), nW, T, H, D, D ** -0.5, L.ptr(out_g), E, L.ptr(lse),
                                             p, L.ptr(seed), L.stream()), 'gather')
    got_g = out_g.float().view(nW, T, H, D).permute(0, 2, 1, 3).cpu().numpy() != 0
    assert np.array_equal(got_g, _padded_mask(sv, full, T, p))
    # gather form with scattered rows: the hash sees token_index rows
    perm = torch.randperm(nW * T, generator=g).int().to(dev)
    qkv_s = torch.empty_like(qkv)
    qkv_s[perm.long()] = qkv
    b = qkv_s.data_ptr()
    out_s = torch.empty((nW * T, E), dtype=torch.bfloat16, device=dev)
    L.check(L.lib.ococc_window_attn_fwd_bf16(b, b + 2 * E, b + 4 * E, 3 * E, 3 * E, 3 * E, L.ptr(perm),
                                             L.ptr(full), nW, T, H, D, D ** -0.5, L.ptr(out_s), E, L.ptr(lse),
                                             p, L.ptr(seed), L.stream()), 'gather')
    got_s = out_s[perm.long()].float().view(nW, T, H, D).permute(0, 2, 1, 3).cpu().numpy() != 0
    rows = perm.cpu().numpy().reshape(nW, T)
    w, h, qi, ki = np.meshgrid(np.arange(nW), np.arange(H), np.arange(T), np.arange(T), indexing='ij')
    assert np.array_equal(got_s, keep(sv, h, rows[w, qi], rows[w, ki], p))
    # p out of range / a missing seed: the library's error return
    for bad_p, bad_seed in ((1.0, seed), (-0.1, seed), (0.1, None)):
        rc = L.lib.ococc_window_attn_fwd_bf16(L.ptr(q), L.ptr(q), L.ptr(v), E, E, E, None, L.ptr(key_len), nW, T, H, D,
                                              D ** -0.5, L.ptr(out), E, L.ptr(lse), bad_p, L.ptr(bad_seed), L.stream())
        assert rc != 0


def test_tile_kernel_mask_is_the_gather_kernels(dev):
    """ococc_window_attn_block_fwd_bf16 with attn_save, Wq = Wk = 0, Wv = I and one-hot x: the saved attention output is
    P_drop"""
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.sst.fused_block import TilePlan, linear_fragments
    g = torch.Generator().manual_seed(5)
    nW, T, p, sv = 40, 16, 0.25, 77777777777
    key_len = _windows(g, nW, T, dev)
    kl = key_len.cpu()
    V = int(kl.sum())
    starts = torch.cumsum(kl, 0) - kl
    tok = torch.full((nW, T), -1, dtype=torch.int32)
    for w in range(nW):
        tok[w, :kl[w]] = torch.arange(int(starts[w]), int(starts[w]) + int(kl[w]))
    tok = tok.view(-1).to(dev)
    x = torch.zeros(V, H, D)
    for w in range(nW):
        for t in range(int(kl[w])):
            x[int(starts[w]) + t, :, t] = 1.0
    x = x.view(V, E).to(dev).bfloat16()
    plan = TilePlan([(tok, key_len, nW, T)], dev)
    w_in = torch.zeros(3 * E, E, device=dev)
    w_in[2 * E:] = torch.eye(E, device=dev)
    wqkv, wo = linear_fragments([w_in, torch.eye(E, device=dev)])
    zb = torch.zeros(3 * E, device=dev)
    ones = torch.ones(E, device=dev)
    y = torch.empty_like(x)
    o = torch.empty_like(x)
    lse = torch.empty((V, H), dtype=torch.float32, device=dev)
    seed = _seed(dev, sv)
    L.check(L.lib.ococc_window_attn_block_fwd_bf16(
        L.ptr(x), None, L.ptr(plan.rows), L.ptr(plan.span), plan.num_tiles, E, H, L.ptr(wqkv), L.ptr(zb), L.ptr(wo),
        L.ptr(zb), L.ptr(ones), L.ptr(zb), 1e-5, L.ptr(y), L.ptr(o), L.ptr(lse), p, L.ptr(seed), L.stream()), 'tile')
    got = o.float().view(V, H, D).cpu().numpy() != 0                     # [query row, head, key slot]
    exp = np.zeros_like(got)
    for w in range(nW):
        n, s0 = int(kl[w]), int(starts[w])
        hh, qi, ki = np.meshgrid(np.arange(H), np.arange(n), np.arange(n), indexing='ij')
        exp[s0:s0 + n, :, :n] = keep(sv, hh, s0 + qi, s0 + ki, p).transpose(1, 0, 2)
    assert np.array_equal(got, exp)
    # the gather kernel on the same rows and seed: the same mask
    qkv = torch.cat([torch.zeros_like(x), torch.zeros_like(x), x], 1).contiguous()
    b = qkv.data_ptr()
    out_g = torch.empty_like(x)
    lse_g = torch.empty((nW, H, T), dtype=torch.float32, device=dev)
    L.check(L.lib.ococc_window_attn_fwd_bf16(b, b + 2 * E, b + 4 * E, 3 * E, 3 * E, 3 * E, L.ptr(tok),
                                             L.ptr(key_len), nW, T, H, D, D ** -0.5, L.ptr(out_g), E,
                                             L.ptr(lse_g), p, L.ptr(seed), L.stream()), 'gather')
    assert np.array_equal(out_g.float().view(V, H, D).cpu().numpy() != 0, got)


def _core_f64(q, k, v, key_len, dout, keep_m, p):
    """oracle/sst_ref.window_attention_core(rounding='window') with the dropout mask [nW, H, T, T] applied: P_drop =
    keep P / (1 - p), rounded to bf16 as the P V and dV operand; dS = P (keep dP / (1 - p) - delta) scale, rounded"""
    nW, T, C = q.shape
    sc = float(D) ** -0.5
    kd = torch.as_tensor(keep_m, device=q.device).double() / (1.0 - float(np.float32(p)))
    q4, k4, v4 = (t.double().view(nW, T, H, D) for t in (q, k, v))
    mask = torch.arange(T, device=q.device)[None, :] >= key_len[:, None].long()
    s = torch.einsum('wthd,wshd->whts', q4, k4) * sc
    s = s.masked_fill(mask[:, None, None, :], float('-inf'))
    pr = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
    pd = _r16(pr * kd)
    o = _r16(torch.einsum('whts,wshd->wthd', pd, v4)).reshape(nW, T, C)
    do4 = dout.double().view(nW, T, H, D)
    delta = (do4 * o.view(nW, T, H, D)).sum(-1)
    dp = torch.einsum('wthd,wshd->whts', do4, v4)
    ds = _r16(pr * (kd * dp - delta.permute(0, 2, 1)[..., None]) * sc)
    dq = _r16(torch.einsum('whts,wshd->wthd', ds, k4)).reshape(nW, T, C)
    dk = _r16(torch.einsum('whts,wthd->wshd', ds, q4)).reshape(nW, T, C)
    dv = _r16(torch.einsum('whts,wthd->wshd', pd, do4)).reshape(nW, T, C)
    return o, dq, dk, dv


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_kernels_vs_float64_with_the_mask(dev, p):
    from objectcentricocccompletion_amd.sst.sst_modules import _WindowAttnCore, _WindowAttnFlat
    g = torch.Generator().manual_seed(11)
    worst = 0.0
    for T in (7, 30, 60, 100, 144):
        nW, sv = 29, 1000 + T
        seed = _seed(dev, sv)
        q, k, v = (torch.randn(nW, T, E, generator=g).to(dev).bfloat16().float().requires_grad_(True) for _ in range(3))
        key_len = _windows(g, nW, T, dev)
        qmask = (torch.arange(T, device=dev)[None, :] < key_len[:, None])[:, :, None]
        dout = torch.randn(nW, T, E, generator=g).to(dev).bfloat16().float() * qmask
        out = _WindowAttnCore.apply(q, k, v, key_len, H, p, seed)
        out.backward(dout)
        km = _padded_mask(sv, key_len, T, p)
        o, dq, dk, dv = _core_f64(q.detach(), k.detach(), v.detach(), key_len, dout, km, p)
        for name, got, exp in (('out', out.detach() * qmask, o * qmask), ('dq', q.grad, dq), ('dk', k.grad, dk),
                               ('dv', v.grad, dv)):
            rel = float((got.double() - exp).norm() / exp.norm())
            worst = max(worst, rel)
            assert rel < 1e-3, ('padded', T, name, rel)
        # gather kernels: the windows' tokens scattered over a flat tensor
        full_rows = int(key_len.sum())
        perm = torch.randperm(full_rows, generator=g).to(dev)
        valid = qmask[..., 0].reshape(-1)
        tok = torch.full((nW * T,), -1, dtype=torch.int32, device=dev)
        tok[valid] = perm.int()
        qkv = torch.empty((full_rows, 3 * E), dtype=torch.bfloat16, device=dev)
        for i, t in enumerate((q, k, v)):
            qkv[perm, i * E:(i + 1) * E] = t.detach().reshape(nW * T, E)[valid].bfloat16()
        qkv.requires_grad_(True)
        of = _WindowAttnFlat.apply(qkv, H, p, seed, tok, key_len, nW, T)
        do_f = torch.empty((full_rows, E), dtype=torch.bfloat16, device=dev)
        do_f[perm] = dout.reshape(nW * T, E)[valid].bfloat16()
        of.backward(do_f)
        rows = tok.view(nW, T).cpu().numpy()
        w, h, qi, ki = np.meshgrid(np.arange(nW), np.arange(H), np.arange(T), np.arange(T), indexing='ij')
        kl = key_len.cpu().numpy()[w]
        km_g = keep(sv, h, rows[w, qi], rows[w, ki], p) & (qi < kl) & (ki < kl)
        o, dq, dk, dv = _core_f64(q.detach(), k.detach(), v.detach(), key_len, dout, km_g, p)
        flat = lambda t: t.reshape(nW * T, E)[valid]
        gq = qkv.grad
        for name, got, exp in (('out', of.detach()[perm], flat(o)), ('dq', gq[perm, :E], flat(dq)),
                               ('dk', gq[perm, E:2 * E], flat(dk)), ('dv', gq[perm, 2 * E:], flat(dv))):
            rel = float((got.double() - exp).norm() / exp.norm())
            worst = max(worst, rel)
            assert rel < 1e-3, ('gather', T, name, rel)
    print(f'p={p}: window attention kernels with dropout vs the rounded float64 chain: worst {worst:.2e}')


def test_dropout_is_unbiased_reproducible_and_seeded(dev):
    from objectcentricocccompletion_amd.sst.sst_modules import _WindowAttnCore
    g = torch.Generator().manual_seed(2)
    nW, T, p = 16, 30, 0.1
    q, k, v = (torch.randn(nW, T, E, generator=g).to(dev).bfloat16().float() for _ in range(3))
    key_len = _windows(g, nW, T, dev)
    qmask = (torch.arange(T, device=dev)[None, :] < key_len[:, None])[:, :, None]
    ref = _WindowAttnCore.apply(q, k, v, key_len, H).double() * qmask
    n = 256
    acc = torch.zeros_like(ref)
    sq = torch.zeros_like(ref)
    for i in range(n):
        o = _WindowAttnCore.apply(q, k, v, key_len, H, p, _seed(dev, 12345 + 7919 * i)).double() * qmask
        acc += o
        sq += o * o
    mean = acc / n
    sem = ((sq / n - mean * mean).clamp(min=0) / n).sqrt()
    # the mean over seeds approaches the p = 0 output within the 1 / sqrt(n) noise (plus the bf16 steps of P and O)
    err = float((mean - ref).norm() / ref.norm())
    noise = float(sem.norm() / ref.norm())
    print(f'mean of {n} dropped outputs vs p = 0: {err:.2e} (standard error {noise:.2e})')
    assert err < 3 * noise + 4e-3
    a = _WindowAttnCore.apply(q, k, v, key_len, H, p, _seed(dev, 99))
    b = _WindowAttnCore.apply(q, k, v, key_len, H, p, _seed(dev, 99))
    c = _WindowAttnCore.apply(q, k, v, key_len, H, p, _seed(dev, 100))
    assert torch.equal(a, b) and not torch.equal(a * qmask, c * qmask)


def test_dropped_fraction_over_a_million_pairs(dev):
    from objectcentricocccompletion_amd import _lib as L
    nW, T, p = 4096, 16, 0.1                 # 4096 windows x 8 heads x 16 x 16 = 8.4e6 live pairs
    q = torch.zeros(nW, T, E, dtype=torch.bfloat16, device=dev)
    v = _one_hot_v(nW, T, dev)
    key_len = torch.full((nW,), T, dtype=torch.int32, device=dev)
    lse = torch.empty((nW, H, T), dtype=torch.float32, device=dev)
    masks = []
    for sv in (31337, 4242424242):
        out = torch.empty_like(q)
        L.check(L.lib.ococc_window_attn_fwd_bf16(L.ptr(q), L.ptr(q), L.ptr(v), E, E, E, None, L.ptr(key_len), nW, T, H, D,
                                                 D ** -0.5, L.ptr(out), E, L.ptr(lse), p, L.ptr(_seed(dev, sv)),
                                                 L.stream()), 'fwd')
        masks.append(out.view(nW, T, H, D).permute(0, 2, 1, 3) == 0)     # dropped [w, h, query, key]
    d1, d2 = masks
    n = d1.numel()
    frac = float(d1.double().mean())
    assert abs(frac - p) < 5 * np.sqrt(p * (1 - p) / n), frac
    s2 = 5 * np.sqrt(p * p * (1 - p * p) / n)
    assert abs(float((d1 & d2).double().mean()) - p * p) < s2
    assert abs(float((d1 & d1.transpose(2, 3)).double().mean()) - (p * p * (T - 1) + p) / T) < s2 + 1e-4


def _scene_args(dev, golden_dir, small_only, training):
    from objectcentricocccompletion_amd.sst import sst_modules as sm
    coors, feats = _scene(golden_dir, small_only)
    inp = sm.SSTInputLayerV2(DROP, WINDOW, SPARSE, shuffle_voxels=False, debug=False, mute=True).eval()
    info = inp(feats.to(dev), coors.to(dev))
    return feats, (info['pos_dict_shift0'], info['flat2win_inds_shift0'], info['key_mask_shift0'])


def _run_layer(enc, feats, args, dy, seed):
    enc.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    x = feats.to(dy.device).requires_grad_(True)
    y = enc(x, *args)
    y.backward(dy)
    return y.detach().float(), x.grad.float(), [p.grad.clone() for p in enc.parameters()]


@pytest.mark.parametrize('small_only', [True, False])
def test_fused_layer_with_dropout_matches_the_operator_path(dev, golden_dir, small_only, monkeypatch):
    """fused tile kernels (+ the per-window kernels of windows above 64 tokens) against the per-operator path with the
    same seed, within the bounds of test_fused_layer_is_bit_reproducible_and_matches_the_operator_path; keep and
    recompute backward modes bitwise; a new seed changes the result"""
    from objectcentricocccompletion_amd.sst import fused_block as fb
    from objectcentricocccompletion_amd.sst import sst_modules as sm
    feats, args = _scene_args(dev, golden_dir, small_only, True)
    enc, _ = _layer(dev, compute_dtype=torch.bfloat16)
    enc.win_attn.self_attn.dropout = 0.1
    enc.train()
    assert enc._fusable()
    g = torch.Generator().manual_seed(8)
    dy = torch.randn(len(feats), 128, generator=g).to(dev).bfloat16()
    keep_run = _run_layer(enc, feats, args, dy, 5)
    again = _run_layer(enc, feats, args, dy, 5)
    monkeypatch.setattr(fb, 'KEEP_ATTENTION', False)
    recompute = _run_layer(enc, feats, args, dy, 5)
    monkeypatch.setattr(fb, 'KEEP_ATTENTION', True)
    for other in (again, recompute):
        assert torch.equal(keep_run[0], other[0]) and torch.equal(keep_run[1], other[1])
        assert all(torch.equal(p, q) for p, q in zip(keep_run[2], other[2]))
    monkeypatch.setattr(sm, 'FUSED_ENCODER_LAYER', False)
    old = _run_layer(enc, feats, args, dy, 5)
    monkeypatch.setattr(sm, 'FUSED_ENCODER_LAYER', True)
    ey, edx = _norm_err(keep_run[0], old[0])[0], _norm_err(keep_run[1], old[1])[0]
    ep = max(_norm_err(p, q)[0] for p, q in zip(keep_run[2], old[2]))
    print(f'fused vs operator path with dropout 0.1 (small windows only: {small_only}): y {ey:.2e}, dx {edx:.2e}, '
          f'parameter gradients worst {ep:.2e}')
    assert ey < 1e-2 and edx < 2e-2 and ep < 3e-2
    other = _run_layer(enc, feats, args, dy, 6)
    assert not torch.equal(keep_run[0], other[0])


def test_eval_mode_is_the_dropout_free_layer(dev, golden_dir):
    """eval() with dropout 0.1 is bitwise the dropout=0.0 module: f32 path, bf16 flat path and fused path"""
    from objectcentricocccompletion_amd.sst import sst_modules as sm
    feats, args = _scene_args(dev, golden_dir, False, False)
    outs = {}
    for name, cfg, fused in (('f32', dict(), True), ('flat', dict(compute_dtype=torch.bfloat16), False),
                             ('fused', dict(compute_dtype=torch.bfloat16), True)):
        res = []
        for drop in (0.1, 0.0):
            enc, _ = _layer(dev, **cfg)
            enc.win_attn.self_attn.dropout = drop
            enc.eval()
            sm.FUSED_ENCODER_LAYER = fused
            try:
                with torch.no_grad():
                    res.append(enc(feats.to(dev), *args).float())
            finally:
                sm.FUSED_ENCODER_LAYER = True
        assert torch.equal(res[0], res[1]), name
        outs[name] = res[0]


def test_graph_captured_layer_draws_a_new_mask_per_replay(dev, golden_dir):
    feats, args = _scene_args(dev, golden_dir, True, True)
    enc, _ = _layer(dev, compute_dtype=torch.bfloat16)
    enc.win_attn.self_attn.dropout = 0.1
    enc.train()
    x = feats.to(dev).requires_grad_(True)
    dy = torch.randn(len(feats), 128, device=dev).bfloat16()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up: plans and caches on the index dict
        for _ in range(2):
            enc(x, *args).backward(dy)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = enc(x, *args)
        y.backward(dy)
    outs = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        outs.append((y.detach().float().clone(), x.grad.float().clone()))
    for yy, gx in outs:
        assert bool(torch.isfinite(yy).all()) and bool(torch.isfinite(gx).all())
    assert not torch.equal(outs[0][0], outs[1][0])
