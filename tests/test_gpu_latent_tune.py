"""The latent-tuning kernels (csrc/latent_tune.hip) and one whole tuning iteration (occ/latent_tune.py) on the MI355X
against the float64 restatement tests/latent_tune_ref.py, at shapes where they can go wrong: 64 k + 27 rows with a second
trip of the row loop and a ragged last tile, 7 RoIs of which one is empty, one RoI owning every row, a one-row segment,
segments that end one row before / on / one row behind the kernels' row strides."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_tune_ref as R   # noqa: E402
from oracle import decoder_ref as D   # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24            # unit round-off of f32
U16 = 2.0 ** -8           # unit round-off of bf16 (8 significant bits, round to nearest even)
EPS = 1e-3
WIDTHS = (512, 1024, 1024)
ROIS, EMPTY_ROI = 7, 3
A_BLOCKS, A_ROWS_PER_BLOCK = 2048, 4                  # kTuneMaxBlocks workgroups of 4 waves, one row per wave and trip
ROWS = 64 * 129 + 27                                  # 8283 = one full trip of kernel A (8192 rows) + 91: 22 workgroups take
assert ROWS > A_BLOCKS * A_ROWS_PER_BLOCK and (ROWS - A_BLOCKS * A_ROWS_PER_BLOCK) % 4 == 3   # a second trip, the last one ragged


@pytest.fixture(autouse=True, scope='module')
def _leave_the_generators_alone():
    """Tests that follow build modules from the process-wide generators: they get the state they would get without this file."""
    import random
    import numpy as np
    state = (random.getstate(), np.random.get_state(), torch.get_rng_state(),
             torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None)
    yield
    random.setstate(state[0])
    np.random.set_state(state[1])
    torch.set_rng_state(state[2])
    if state[3] is not None:
        torch.cuda.set_rng_state_all(state[3])


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def sorted_index(rows, g, rois=ROIS, empty=EMPTY_ROI):
    idx = torch.randint(0, rois - 1, (rows,), generator=g).sort().values
    return (idx + (idx >= empty)).int()


@pytest.fixture(scope='module')
def fwd(dev):
    """One training-forward launch on ROWS rows: the stored z / statistics / logits that the backward kernels read."""
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ import fused_mlp as fm
    g = torch.Generator().manual_seed(ROWS)
    W = [torch.randn(n, k, generator=g) / k ** 0.5 for k, n in ((60, 512), (512, 1024), (1024, 1024))]
    gam = [(1 + 0.2 * torch.randn(n, generator=g)).to(dev) for n in WIDTHS]
    bet = [(0.2 * torch.randn(n, generator=g)).to(dev) for n in WIDTHS]
    hw, hb = (torch.randn(1024, generator=g) / 32).to(dev), torch.tensor([-0.1]).to(dev)
    xyz = (torch.rand(ROWS, 3, generator=g) * 2 - 1) * torch.tensor([8., 8., 4.])
    add = torch.randn(ROIS, 512, generator=g).to(dev)
    idx = sorted_index(ROWS, g).to(dev)
    pe = fm.pos_encode_bf16(xyz.to(dev), 10, [-8.0, -8.0, -4.0, 8.0, 8.0, 4.0])
    frags = fm.linear_fragments32([w.to(dev) for w in W], [64, 512, 1024])
    zs = [torch.empty((ROWS, n), dtype=torch.bfloat16, device=dev) for n in WIDTHS]
    ys = [torch.empty((ROWS, n), dtype=torch.bfloat16, device=dev) for n in WIDTHS]
    st = [torch.empty((ROWS, 2), dtype=torch.float32, device=dev) for _ in WIDTHS]
    out = torch.empty((ROWS,), dtype=torch.float32, device=dev)
    vp = lambda ts: (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts])
    L.check(L.lib.ococc_occ_mlp_train_fwd_bf16(L.ptr(pe), ROWS, L.ptr(add), L.ptr(idx), vp(frags), vp(gam), vp(bet), EPS,
                                               L.ptr(hw), L.ptr(hb), 0, None, vp(zs), vp(ys), vp(st), L.ptr(out), L.stream()),
            'occ_mlp_train_fwd')
    torch.cuda.synchronize()
    lab = (torch.rand(ROWS, generator=g) < 0.5).int().to(dev)
    wts = (torch.rand(ROWS, generator=g) + 0.5).to(dev)
    return dict(z=zs, stats=st, logits=out, gam=gam, bet=bet, hw=hw, idx=idx, labels=lab, weights=wts)


def run_a(f, logits, labels, weights, scale, rows=ROWS, pad=64):
    from objectcentricocccompletion_amd import _lib as L
    dev = logits.device
    dz = torch.full((rows + pad, 1024), 0x5A3C, dtype=torch.int16, device=dev).view(torch.bfloat16)
    L.check(L.lib.ococc_occ_tune_head_lnbwd_bf16(L.ptr(logits), L.ptr(labels), L.ptr(weights), scale, L.ptr(f['hw']),
                                                 L.ptr(f['z'][2]), L.ptr(f['stats'][2]), L.ptr(f['gam'][2]),
                                                 L.ptr(f['bet'][2]), rows, 1024, L.ptr(dz), L.stream()), 'tune_head_lnbwd')
    torch.cuda.synchronize()
    assert bool((bits(dz[rows:]) == 0x5A3C).all()), 'written behind the last row'
    return dz[:rows]


@pytest.mark.parametrize('weighted', [False, True], ids=['unweighted', 'weighted'])
@pytest.mark.parametrize('labels', ['zeros', 'ones', 'mixed'])
def test_head_lnbwd_vs_float64(dev, fwd, labels, weighted):
    """Kernel A against float64 from the same stored z2 / statistics.  dz_c = rstd (t_c - s1 - xhat_c s2), t_c = d hw_c G_c g_c,
    G = GELU'(xhat g + b), s1 = mean t, s2 = mean (t xhat), d = scale w (sigmoid(logit) - label).  In f32 (u = 2^-24):
      * d: exp, the division and the subtraction leave an ABSOLUTE error of at most 4 u in sigmoid - label (the difference
        cancels when the sigmoid saturates towards the label), two more roundings for scale and w:
        |d^ - d| <= 4 u scale w + 2 u |d| -- 8 u scale w + 2 u |d| is allowed;
      * xhat: two roundings; the argument of G: three more, |G''| <= 0.8, |g| <= 2, |b| <= 1: G moves by at most
        0.8 * 3 u (2 |xhat| + 1); its own approximation error is 1.9e-7 = 3.2 u (ln_math.hpp), v_exp / v_rcp a few u more:
        |G^ - G| <= 32 u (1 + |xhat|); the three products of t: 3 u |t|, and |G| <= 1.13;
      * s1, s2: any order of summing N = 1024 f32 numbers is within (N - 1) u sum |t_i|; the last three operations 3 u.
    With a_c = |hw_c g_c| and unit_c = rstd (a_c + mean a + |xhat_c| mean (a |xhat|)) (latent_tune_ref.head_lnbwd) every
    term is at most 1200 u |d| unit_c for |xhat| <= 32 = sqrt(N), so the f32 value is within
        E32 = (1200 u |d| + 8 u scale w) unit_c
    of float64, and the bf16 store (round to nearest, u16 = 2^-8) adds u16 (|dz| + E32):
        |dz^ - dz| <= u16 |dz| + (1 + u16) E32."""
    f = fwd
    lab = {'zeros': torch.zeros_like(f['labels']), 'ones': torch.ones_like(f['labels']), 'mixed': f['labels']}[labels]
    w = f['weights'] if weighted else None
    scale = 0.7 / ROWS
    got = run_a(f, f['logits'], lab, w, scale).double()
    ref = R.head_lnbwd(f['logits'], lab, w, scale, f['hw'], f['z'][2], f['stats'][2][:, 0], f['stats'][2][:, 1],
                       f['gam'][2], f['bet'][2])
    ww = torch.ones_like(ref['d']) if w is None else w.double()
    e32 = (1200 * U * ref['d'].abs() + 8 * U * scale * ww)[:, None] * ref['unit']
    bound = U16 * ref['dz'].abs() + (1 + U16) * e32
    err = (got - ref['dz']).abs()
    worst = float((err / bound).max())
    rel = float((got - ref['dz']).norm() / ref['dz'].norm())
    print(f'kernel A labels {labels} weighted {weighted}: largest error / bound {worst:.4f}, norm-wise error {rel:.3e}')
    assert float(ref['dz'].abs().max()) > 0 and bool(torch.isfinite(got).all())
    assert bool((err <= bound).all()), worst
    # the second trip and the ragged tile were written by the formula too (covered above); the same launch again: same bits
    assert torch.equal(bits(run_a(f, f['logits'], lab, w, scale)), bits(got.to(torch.bfloat16)))


def test_head_lnbwd_saturated_logits_and_few_rows(dev, fwd):
    """logits of +-30 (and far beyond: exp overflows) give finite gradients within the same bound; 1, 3 and 5 rows."""
    f = fwd
    scale = 1.0 / 64
    logits = f['logits'].clone()
    logits[0::4], logits[1::4] = 30.0, -30.0
    logits[2], logits[6] = 800.0, -800.0
    for rows in (ROWS, 1, 3, 5):
        got = run_a(f, logits, f['labels'], None, scale, rows=rows).double()
        assert bool(torch.isfinite(got).all())
        if rows == ROWS:
            # saturated on the side of its label: the gradient vanishes (|d| <= 1e-13 scale); on the other side |d| = scale
            sat = logits.abs() >= 30
            agree = sat & ((logits > 0) == (f['labels'] > 0))
            assert bool(agree.any()) and bool((sat & ~agree).any())
            assert float(got[agree].abs().max()) <= 1e-10 * scale < float(got[sat & ~agree].abs().max())
        ref = R.head_lnbwd(logits[:rows], f['labels'][:rows], None, scale, f['hw'], f['z'][2][:rows], f['stats'][2][:rows, 0],
                           f['stats'][2][:rows, 1], f['gam'][2], f['bet'][2])
        e32 = (1200 * U * ref['d'].abs() + 8 * U * scale)[:, None] * ref['unit']
        bound = U16 * ref['dz'].abs() + (1 + U16) * e32
        err = (got - ref['dz']).abs()
        assert bool((err <= bound).all()), (rows, float((err / bound).max()))


def run_b(x, idx, K):
    from objectcentricocccompletion_amd import _lib as L
    out = torch.full((K + 2, 512), float('nan'), dtype=torch.float32, device=x.device)
    L.check(L.lib.ococc_segment_sum_bf16(L.ptr(x), L.ptr(idx), x.size(0), 512, L.ptr(out), K, L.stream()), 'segment_sum')
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[K:]).all()), 'written behind the last segment'
    return out[:K]


def _index_from_counts(counts, dev):
    return torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts)).int().to(dev)


# kernel B takes 32 rows of a segment per trip (4 waves of 8 rows): extents one short of, on and one past that stride
B_CASES = {
    'seven-rois-one-empty': None,
    'one-roi-owns-all': [0, ROWS, 0],
    'one-row-segments': [1, 1, 0, 1, ROWS - 3],
    'stride-edges': [31, 32, 33, 0, 63, 64, 65, 1, 127, 129, 7, ROWS - 31 - 32 - 33 - 63 - 64 - 65 - 1 - 127 - 129 - 7],
    'leading-and-trailing-empty': [0, 0, 40, ROWS - 40, 0, 0],
}


@pytest.mark.parametrize('case', list(B_CASES))
def test_segment_sum_vs_float64(dev, fwd, case):
    """Kernel B against the float64 sum of the same bf16 values.  Whatever the order, summing n f32 numbers is within
    (n - 1) u sum |x_i| of the exact sum (u = 2^-24; additions to a zero accumulator are exact): 0 for a one-row segment."""
    g = torch.Generator().manual_seed(len(case))
    x = (torch.randn(ROWS, 512, generator=g) * torch.rand(ROWS, 1, generator=g) * 4).to(dev).to(torch.bfloat16)
    counts = B_CASES[case]
    idx = fwd['idx'] if counts is None else _index_from_counts(counts, dev)
    K = ROIS if counts is None else len(counts)
    assert idx.numel() == ROWS and bool((idx[1:] >= idx[:-1]).all())
    got = run_b(x, idx, K)
    ref, ref_abs, n = R.segment_sum(x, idx, K)
    bound = (n.double() - 1).clamp(min=0)[:, None] * U * ref_abs
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print(f'kernel B {case}: rows per segment {n.tolist()}, largest error {float(err.max()):.3e}, / bound {ratio:.4f}')
    assert bool((err <= bound).all()), ratio
    empty = n == 0
    assert bool(empty.any()) and bool((bits(got[empty]) == 0).all())          # exactly +0, not merely small
    assert bool((got[n == 1].double() == ref[n == 1]).all())
    assert torch.equal(bits(run_b(x, idx, K)), bits(got))                      # no atomics: two runs, equal bits
    # rows whose index is outside [0, K) are left out; fewer segments than the indices name
    got2 = run_b(x, idx, K - 1)
    assert torch.equal(bits(got2), bits(got[:K - 1]))


def test_segment_sum_no_rows(dev):
    from objectcentricocccompletion_amd import _lib as L
    out = torch.full((3, 512), float('nan'), dtype=torch.float32, device=dev)
    L.check(L.lib.ococc_segment_sum_bf16(None, None, 0, 512, L.ptr(out), 3, L.stream()), 'segment_sum')
    torch.cuda.synchronize()
    assert bool((bits(out) == 0).all())


SEED = 5


@pytest.mark.parametrize('use_ln', [True, False], ids=['ln', 'no-ln'])
@pytest.mark.parametrize('D_', [1536, 192])
def test_latent_ln_adam_vs_float64_and_torch(dev, D_, use_ln):
    """Kernel C over 5 steps (StepLR with step_size 3: the learning rate drops in front of the fourth) from random e and
    d_n, against float64 (latent_tune_ref.latent_ln_adam) -- and torch's own f32 layer_norm backward + torch.optim.Adam +
    StepLR against the same float64: per row and per tensor (e, m, v),
        max_c |kernel - f64| <= 2 max_c |torch - f64| + 2^-23 max_c |value|
    (the factor: another order of the row reductions; 2^-23 |value|: one f32 ulp).  Row 2 has a zero gradient in every step:
    its e stays bit-unchanged.  Precondition (change SEED if it fails): no |de| below 1e-4 of its row's rms, so that the
    first step, lr * sign(de) per coordinate, cannot flip on rounding (later steps move by the running mean m, which a
    coordinate next to zero changes by next to nothing)."""
    K, steps, lr, step_size, gamma_lr, b1, b2, eps, ln_eps = 7, 5, 0.01, 3, 0.1, 0.9, 0.999, 1e-8, 1e-5
    from objectcentricocccompletion_amd import _lib as L
    g = torch.Generator().manual_seed(SEED + D_)
    e0 = torch.randn(K, D_, generator=g) * 1.5 + 0.3
    dns = [torch.randn(K, D_, generator=g) * 10.0 ** float(torch.randint(-6, 0, (1,), generator=g)) for _ in range(steps)]
    for d in dns:
        d[2] = 0
    ln_g, ln_b = 1 + 0.2 * torch.randn(D_, generator=g), 0.2 * torch.randn(D_, generator=g)
    # float64
    e64, m64, v64 = e0.double(), torch.zeros(K, D_, dtype=torch.float64), torch.zeros(K, D_, dtype=torch.float64)
    ref = []
    for t in range(1, steps + 1):
        e64, m64, v64, de = R.latent_ln_adam(e64, dns[t - 1], m64, v64, ln_g, ln_eps, use_ln,
                                             R.step_lr(lr, step_size, gamma_lr, t - 1), b1, b2, eps, t)
        if t == 1:
            live = torch.arange(K) != 2
            rms = de[live].pow(2).mean(1, keepdim=True).sqrt()
            assert float((de[live].abs() / rms).min()) >= 1e-4, 'change SEED: a gradient coordinate next to zero'
        ref.append((e64, m64, v64))
    # torch in f32 on the device
    p = e0.to(dev).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size, gamma_lr)
    tor = []
    for t in range(1, steps + 1):
        opt.zero_grad()
        if use_ln:
            torch.nn.functional.layer_norm(p, (D_,), ln_g.to(dev), ln_b.to(dev), ln_eps).backward(dns[t - 1].to(dev))
        else:
            p.grad = dns[t - 1].to(dev).clone()
        opt.step()
        sched.step()
        s = opt.state[p]
        tor.append((p.detach().clone(), s['exp_avg'].clone(), s['exp_avg_sq'].clone()))
    # the kernel
    e = e0.to(dev).clone()
    m, v = torch.zeros_like(e), torch.zeros_like(e)
    gam = ln_g.to(dev)
    worst = {}
    for t in range(1, steps + 1):
        dn = dns[t - 1].to(dev)
        de = torch.empty_like(e)
        L.check(L.lib.ococc_latent_ln_adam_f32(L.ptr(e), L.ptr(dn), L.ptr(m), L.ptr(v), K, D_, L.ptr(gam) if use_ln else None,
                                               ln_eps, int(use_ln), lr * gamma_lr ** ((t - 1) // step_size), b1, b2, eps, t,
                                               L.ptr(de), L.stream()), 'latent_ln_adam')
        torch.cuda.synchronize()
        assert torch.equal(bits(e[2]), bits(e0[2].to(dev))), t
        for name, got, r64, t32 in zip('emv', (e, m, v), ref[t - 1], tor[t - 1]):
            r64 = r64.to(dev)
            ek = (got.double() - r64).abs().amax(1)
            et = (t32.double() - r64).abs().amax(1)
            tol = 2 * et + 2.0 ** -23 * r64.abs().amax(1)
            worst[name] = max(worst.get(name, (0.0, 0.0, 0.0)), (float(ek.max()), float(et.max()), float((ek / tol.clamp(min=1e-300)).max())))
            assert bool((ek <= tol).all()), (name, t, ek.tolist(), et.tolist())
    print(f'kernel C D {D_} use_ln {use_ln}: largest error against float64 over 5 steps (kernel, torch f32, kernel / allowed) '
          + ', '.join(f'{k}: {a:.3e} {b:.3e} {c:.3f}' for k, (a, b, c) in worst.items()))
    assert float((e[0] - e0[0].to(dev)).abs().min()) > 0   # every coordinate of a live row moved


def _decoder(dev):
    from objectcentricocccompletion_amd.occ.occ_base import OccDecoder
    torch.manual_seed(3)
    dec = OccDecoder(1536, [512, 1024, 1024], pos_encode_L=10, norm_cfg=dict(type='LN', eps=EPS), act='gelu', occ_dropout=0.0,
                     use_ln=True).to(dev).eval()
    with torch.no_grad():   # (LayerNorm parameters away from their 1 / 0 initial values)
        g = torch.Generator().manual_seed(8)
        for mod in dec.modules():
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.copy_((1 + 0.2 * torch.randn(mod.weight.shape, generator=g)).to(dev))
                mod.bias.copy_((0.2 * torch.randn(mod.bias.shape, generator=g)).to(dev))
    dec.compute_dtype = torch.bfloat16
    for p in dec.parameters():
        p.requires_grad = False
    return dec


@pytest.mark.parametrize('weighted', [False, True], ids=['unweighted', 'weighted'])
def test_first_iteration_gradient_vs_float64_autograd(dev, weighted):
    """The latent gradient of tune_latents' first iteration against float64 autograd through oracle/decoder_ref.py with
    rounding='train' (the kernels' own positional encoding as input); per RoI
        |de - de64| / |de64| <= 1.25 err_autograd + 1e-6,
    err_autograd the same error of the existing bf16 autograd path (OccDecoder.forward with a latent that requires a
    gradient: _OccMlpTrain), which rounds the loss gradient twice (d, then d * head_w) where kernel A rounds once (dz2).
    Measured on the MI355X, per RoI: kernels 0.85e-3 .. 1.9e-3, bf16 autograd 1.8e-3 .. 2.4e-3 (weighted: 0.86e-3 .. 2.0e-3
    against 1.8e-3 .. 2.9e-3)."""
    from objectcentricocccompletion_amd.occ import fused_mlp as fm, latent_tune
    dec = _decoder(dev)
    M = 64 * 9 + 27
    g = torch.Generator().manual_seed(21)
    e0 = (torch.randn(ROIS, 1536, generator=g)).to(dev)
    xyz = ((torch.rand(M, 3, generator=g) * 2 - 1) * torch.tensor([8., 8., 4.])).to(dev)
    idx = sorted_index(M, g).to(dev)
    labels = (torch.rand(M, generator=g) < 0.4).long().to(dev)
    w = (torch.rand(M, generator=g) + 0.5).to(dev) if weighted else None
    tuned, info = latent_tune.tune_latents(dec, e0, xyz, labels, idx.long(), 1, weights=w, debug=True)
    torch.cuda.synchronize()
    de = info['de'].double()
    # existing bf16 autograd path
    r = e0.clone().requires_grad_(True)
    with torch.enable_grad():
        logits = dec(r, xyz, idx.long()).view(-1)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels.float(), reduction='none')
        (loss if w is None else loss * w).mean().backward()
    dl = float((logits.detach() - info['logits']).abs().max())
    print(f'logits of the two paths differ by at most {dl:.3e}')
    assert dl <= 2e-2          # the same forward launch on the same inputs (roi_part: the same GEMM, into a given buffer)
    auto = r.grad.double()
    # float64
    layers, head = dec._fused_layers()
    P = dict(W_roi=layers[0][0].weight[:, :1536], W_pe=layers[0][0].weight[:, 1536:], W1=layers[1][0].weight,
             W2=layers[2][0].weight, g=[ln.weight for _, ln in layers], b=[ln.bias for _, ln in layers],
             hw=head.weight.view(-1), hb=head.bias, eps=EPS, use_ln=True, ln_g=dec.ln.weight, ln_b=dec.ln.bias, ln_eps=dec.ln.eps)
    pe = fm.pos_encode_bf16(xyz, 10, dec.pos_encode.norm_bound)[:, :60]
    q = e0.double().clone().requires_grad_(True)
    n = D.layer_norm(q, P['ln_g'], P['ln_b'], P['ln_eps'])
    roi_part = n @ P['W_roi'].double().t()
    roi_part = roi_part + (roi_part.detach().float().double() - roi_part.detach())     # f32 in the product, straight-through
    x, out = pe, None
    for l, W in enumerate((P['W_pe'], P['W1'], P['W2'])):
        x, out = D.mlp_layer(x, W, P['g'][l], P['b'][l], EPS, add=roi_part if l == 0 else None, idx=idx if l == 0 else None,
                             head_w=P['hw'] if l == 2 else None, head_b=P['hb'] if l == 2 else None, rounding='train')[:2]
    l64 = torch.nn.functional.binary_cross_entropy_with_logits(out, labels.double(), reduction='none')
    (l64 if w is None else l64 * w.double()).mean().backward()
    ref = q.grad
    # ... which the hand-written float64 iteration reproduces
    hand = R.latent_gradient(P, pe, e0, idx, labels, w, 1.0, rounding='train')[0]
    assert float((hand - ref).abs().max()) <= 1e-10 * float(ref.abs().max())
    live = torch.arange(ROIS, device=dev) != EMPTY_ROI
    assert bool((ref[EMPTY_ROI] == 0).all()) and bool((de[EMPTY_ROI] == 0).all()) and bool((auto[EMPTY_ROI] == 0).all())
    ek = ((de - ref).norm(dim=1) / ref.norm(dim=1).clamp(min=1e-300))[live]
    ea = ((auto - ref).norm(dim=1) / ref.norm(dim=1).clamp(min=1e-300))[live]
    print(f'first iteration, weighted {weighted}: per RoI relative error of de, kernels {[f"{v:.2e}" for v in ek.tolist()]}, '
          f'bf16 autograd {[f"{v:.2e}" for v in ea.tolist()]}')
    assert bool((ek <= 1.25 * ea + 1e-6).all()), (ek.tolist(), ea.tolist())
    # the tuned latent: Adam's first step, at most lr per coordinate, none for the RoI without rows
    moved = (tuned - e0).abs()
    assert bool((moved[EMPTY_ROI] == 0).all()) and float(moved[live].max()) <= 0.01 * (1 + 1e-5)


def test_occ_mlp_train_skips_gradients_nobody_asked_for(dev, fwd):
    """_OccMlpTrain with only roi_part requiring a gradient: d_roi bit-equal to the run in which everything requires one,
    no gradient handed to the frozen parameters."""
    from objectcentricocccompletion_amd.occ import fused_mlp as fm
    rows = 64 * 3 + 27
    g = torch.Generator().manual_seed(5)
    W = [(torch.randn(n, k, generator=g) / k ** 0.5).to(dev) for k, n in ((60, 512), (512, 1024), (1024, 1024))]
    hw, hb = (torch.randn(1, 1024, generator=g) / 32).to(dev), torch.tensor([-0.1]).to(dev)
    add = torch.randn(ROIS, 512, generator=g).to(dev)
    xyz = ((torch.rand(rows, 3, generator=g) * 2 - 1) * torch.tensor([8., 8., 4.])).to(dev)
    pe = fm.pos_encode_bf16(xyz, 10, [-8.0, -8.0, -4.0, 8.0, 8.0, 4.0])
    idx = sorted_index(rows, g).to(dev)
    dl = torch.randn(rows, 1, generator=g).to(dev)
    grads = []
    for everything in (True, False):
        leaf = lambda t, on: t.detach().clone().requires_grad_(on)
        roi = leaf(add, True)
        ps = [leaf(t, everything) for t in (*W, *fwd['gam'], *fwd['bet'], hw, hb)]
        out = fm.occ_mlp_train(pe, roi, idx, ps[0], ps[1], ps[2], ps[3:6], ps[6:9], EPS, ps[9], ps[10], 0, (0, 0, 0),
                               fm.DecoderWeights())
        out.backward(dl)
        torch.cuda.synchronize()
        grads.append((roi.grad.clone(), [p.grad for p in ps]))
    assert torch.equal(bits(grads[0][0]), bits(grads[1][0])) and float(grads[0][0].abs().max()) > 0
    assert all(gr is not None for gr in grads[0][1]) and all(gr is None for gr in grads[1][1])
