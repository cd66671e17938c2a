"""Latent tuning without a GPU: the three exports of csrc/latent_tune.hip and their argument checks, the float64
reference (tests/latent_tune_ref.py) against torch's float64 autograd + torch.optim.Adam / StepLR, and the head's
online_tuning on an empty sample."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_tune_ref as R   # noqa: E402
from oracle import decoder_ref as D   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ococc_occ_tune_head_lnbwd_bf16', 'ococc_segment_sum_bf16', 'ococc_latent_ln_adam_f32')
OCOCC_OK, OCOCC_EINVAL = 0, -1


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


def test_exports_declared_bound_and_documented():
    from objectcentricocccompletion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ococc_hip.h')).read()
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    makefile = open(os.path.join(ROOT, 'objectcentricocccompletion_amd', 'csrc', 'Makefile')).read()
    assert 'latent_tune.hip' in makefile
    for name in NAMES:
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES and name in integration, name
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, header)
        assert m, name
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name


def test_argument_errors_are_codes():
    """No launch is reached: pointers are placeholders that are never dereferenced."""
    from objectcentricocccompletion_amd import _lib
    lib, p = _lib.lib, 4096
    assert _lib.lib.ococc_last_error is not None
    # zero rows: OCOCC_OK without a launch, pointers not looked at
    assert lib.ococc_occ_tune_head_lnbwd_bf16(None, None, None, 1.0, None, None, None, None, None, 0, 1024, None, None) == OCOCC_OK
    assert lib.ococc_segment_sum_bf16(None, None, 0, 512, None, 0, None) == OCOCC_OK
    assert lib.ococc_latent_ln_adam_f32(None, None, None, None, 0, 1536, None, 1e-5, 1, 0.01, 0.9, 0.999, 1e-8, 1, None, None) == OCOCC_OK
    # channel counts
    for c in (512, 1023, 2048, 0):
        assert lib.ococc_occ_tune_head_lnbwd_bf16(p, p, None, 1.0, p, p, p, p, p, 8, c, p, None) == OCOCC_EINVAL, c
        assert b'1024' in lib.ococc_last_error()
    for c in (1024, 511, 64, 0):
        assert lib.ococc_segment_sum_bf16(p, p, 8, c, p, 3, None) == OCOCC_EINVAL, c
        assert b'512' in lib.ococc_last_error()
    # D out of range or not a multiple of 4
    for d in (0, 2, 1538, 2052, 4096, -4):
        assert lib.ococc_latent_ln_adam_f32(p, p, p, p, 2, d, p, 1e-5, 1, 0.01, 0.9, 0.999, 1e-8, 1, None, None) == OCOCC_EINVAL, d
    assert lib.ococc_latent_ln_adam_f32(p, p, p, p, 2, 1536, p, 1e-5, 1, 0.01, 0.9, 0.999, 1e-8, 0, None, None) == OCOCC_EINVAL  # t from 1
    # null pointers
    args = [p, p, None, 1.0, p, p, p, p, p, 8, 1024, p, None]
    for i in (0, 1, 4, 5, 6, 7, 8, 11):
        a = list(args)
        a[i] = None
        assert lib.ococc_occ_tune_head_lnbwd_bf16(*a) == OCOCC_EINVAL, i
        assert b'null' in lib.ococc_last_error()
    for a in ([None, p, 8, 512, p, 3, None], [p, None, 8, 512, p, 3, None], [p, p, 8, 512, None, 3, None]):
        assert lib.ococc_segment_sum_bf16(*a) == OCOCC_EINVAL
    args = [p, p, p, p, 2, 1536, p, 1e-5, 1, 0.01, 0.9, 0.999, 1e-8, 1, None, None]
    for i in (0, 1, 2, 3, 6):
        a = list(args)
        a[i] = None
        assert lib.ococc_latent_ln_adam_f32(*a) == OCOCC_EINVAL, i
    # negative sizes
    assert lib.ococc_occ_tune_head_lnbwd_bf16(p, p, None, 1.0, p, p, p, p, p, -1, 1024, p, None) == OCOCC_EINVAL
    assert lib.ococc_segment_sum_bf16(p, p, -1, 512, p, 3, None) == OCOCC_EINVAL
    assert lib.ococc_latent_ln_adam_f32(p, p, p, p, -1, 1536, p, 1e-5, 1, 0.01, 0.9, 0.999, 1e-8, 1, None, None) == OCOCC_EINVAL


def _case(use_ln, K=3, M=40, Dl=24, seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    P = dict(W_roi=rn(512, Dl) / Dl ** 0.5, W_pe=rn(512, 60) / 60 ** 0.5, W1=rn(1024, 512) / 512 ** 0.5,
             W2=rn(1024, 1024) / 32, g=[1 + 0.2 * rn(n) for n in (512, 1024, 1024)], b=[0.2 * rn(n) for n in (512, 1024, 1024)],
             hw=rn(1024) / 32, hb=torch.tensor([-0.1], dtype=torch.float64), eps=1e-3, use_ln=use_ln,
             ln_g=1 + 0.2 * rn(Dl), ln_b=0.2 * rn(Dl), ln_eps=1e-5)
    xyz = (torch.rand(M, 3, generator=g) * 2 - 1) * torch.tensor([8., 8., 4.])
    pe = D.pos_encode(xyz).double()
    idx = torch.sort(torch.randint(0, K, (M,), generator=g)).values
    labels = torch.randint(0, 2, (M,), generator=g)
    weights = torch.rand(M, generator=g, dtype=torch.float64) + 0.5
    return P, pe, rn(K, Dl), idx, labels, weights


def _autograd_forward(P, pe, e, idx, rounding):
    n = D.layer_norm(e, P['ln_g'], P['ln_b'], P['ln_eps']) if P['use_ln'] else e
    roi_part = n @ P['W_roi'].t()
    if rounding == 'train':
        # (straight-through: a cast to float32 inside the graph would round the GRADIENT to float32 on its way back)
        roi_part = roi_part + (roi_part.detach().to(torch.float32).to(torch.float64) - roi_part.detach())
    x, head = pe, None
    for l, W in enumerate((P['W_pe'], P['W1'], P['W2'])):
        x, head = D.mlp_layer(x, W, P['g'][l], P['b'][l], P['eps'], add=roi_part if l == 0 else None,
                              idx=idx if l == 0 else None, head_w=P['hw'] if l == 2 else None,
                              head_b=P['hb'] if l == 2 else None, rounding=rounding)[:2]
    return head


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('use_ln', [True, False])
def test_reference_iteration_equals_float64_autograd_and_adam(use_ln, weighted):
    """3 RoIs, 40 rows, 3 iterations, StepLR stepping after the second: the hand-written float64 iteration against
    torch's float64 autograd through the same forward + torch.optim.Adam + StepLR, to 1e-12."""
    P, pe, e0, idx, labels, weights = _case(use_ln)
    w = weights if weighted else None
    lw, iters = 0.7, 3
    got, des = R.tune(P, pe, e0, idx, labels, w, iters, lr=0.01, step_size=2, gamma=0.1, loss_weight=lw)
    e = e0.clone().requires_grad_(True)
    opt = torch.optim.Adam([e], lr=0.01)
    sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.1)
    for it in range(iters):
        opt.zero_grad()
        logits = _autograd_forward(P, pe, e, idx, None)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels.double(), reduction='none')
        loss = (lw * (loss if w is None else loss * w)).mean()
        loss.backward()
        assert float((des[it] - e.grad).abs().max()) <= 1e-12 * max(1.0, float(e.grad.abs().max())), it
        opt.step()
        sched.step()
    assert float((got - e.detach()).abs().max()) <= 1e-12
    assert float((got - e0).abs().min()) > 1e-3          # every coordinate moved (Adam's first steps are lr-sized)


def test_reference_gradient_with_training_roundings():
    """rounding='train': the hand-written backward reads the rounded z, its statistics and the rounded operand weights,
    every rounding straight-through -- the float64 autograd of oracle/decoder_ref.py's forward with r16_ste."""
    P, pe, e0, idx, labels, weights = _case(True, seed=3)
    pe = D.r16(pe)
    de, _, logits = R.latent_gradient(P, pe, e0, idx, labels, weights, 1.0, rounding='train')
    e = e0.clone().requires_grad_(True)
    out = _autograd_forward(P, pe, e, idx, 'train')
    assert float((out.detach() - logits).abs().max()) <= 1e-12
    loss = (torch.nn.functional.binary_cross_entropy_with_logits(out, labels.double(), reduction='none') * weights).mean()
    loss.backward()
    assert float((de - e.grad).abs().max()) <= 1e-12 * max(1.0, float(e.grad.abs().max()))


def test_reference_pieces():
    g = torch.Generator().manual_seed(1)
    # loss gradient at saturated logits: finite, the exact tails
    d = R.loss_grad(torch.tensor([30.0, -30.0, 30.0, -30.0, 800.0, -800.0]), torch.tensor([1, 0, 0, 1, 1, 0]), None, 1.0)
    assert bool(torch.isfinite(d).all())
    assert abs(float(d[0]) + 9.357622968839299e-14) < 1e-25 and abs(float(d[1]) - 9.357622968839299e-14) < 1e-25
    assert abs(float(d[2]) - 1.0) < 1e-12 and abs(float(d[3]) + 1.0) < 1e-12 and float(d[4]) == 0.0 and float(d[5]) == 0.0
    # segment sum: empty segment, out-of-range rows left out
    x = torch.randn(9, 4, generator=g, dtype=torch.float64)
    idx = torch.tensor([-1, 0, 0, 2, 2, 2, 3, 5, 7])
    s, sa, cnt = R.segment_sum(x, idx, 6)
    assert cnt.tolist() == [2, 0, 3, 1, 0, 1] and bool((s[1] == 0).all()) and torch.equal(s[2], x[3:6].sum(0))
    assert torch.equal(sa[0], x[1:3].abs().sum(0))
    # a zero gradient row does not move under Adam, with and without the LayerNorm
    e = torch.randn(2, 8, generator=g, dtype=torch.float64)
    dn = torch.randn(2, 8, generator=g, dtype=torch.float64)
    dn[1] = 0
    for use_ln in (True, False):
        e1, m1, v1, de = R.latent_ln_adam(e, dn, torch.zeros_like(e), torch.zeros_like(e), torch.ones(8), 1e-5, use_ln,
                                          0.01, 0.9, 0.999, 1e-8, 1)
        assert torch.equal(e1[1], e[1]) and bool((m1[1] == 0).all()) and bool((v1[1] == 0).all())
        assert float((e1[0] - e[0]).abs().min()) > 0.009      # first Adam step: lr * sign(de)


def _cpu_head():
    from objectcentricocccompletion_amd import heads  # noqa: F401
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import HEADS
    cfg = ococcnet_model_cfg()
    hc = dict(cfg['roi_head']['bbox_head'])
    hc['train_cfg'], hc['test_cfg'] = cfg['train_cfg'], cfg['test_cfg']
    return HEADS.build(hc).eval()


def test_online_tuning_on_an_empty_sample_returns_its_input():
    head = _cpu_head()
    assert callable(head.online_tuning)
    latent = torch.randn(4, head.roi_feature_channels)
    rois = torch.tensor([[0, 0, 0, 0, 2.0, 4.0, 1.5, 0.1]] * 4)
    with torch.no_grad():
        out = head.online_tuning(latent, torch.zeros(0, 3), rois, torch.zeros(0, dtype=torch.long), downsample_size=16,
                                 balance_sample=True, num_iter=3)
    assert out is latent
    out = head.online_tuning(latent[:0], torch.zeros(0, 3), rois[:0], torch.zeros(0, dtype=torch.long))
    assert out.shape == (0, head.roi_feature_channels)


def test_tools_test_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location('ococc_tools_test', os.path.join(ROOT, 'tools', 'test.py'))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    a = t.parse_args(['cfg.py', 'ck.pth', '--eval', 'iou', '--online-tuning', '3', '--decoder-dtype', 'bf16'])
    assert a.online_tuning == 3 and a.tuning_samples is None and a.decoder_dtype == 'bf16'
    a = t.parse_args(['cfg.py', 'ck.pth', '--eval', 'iou', '--online-tuning', '3', '--tuning-samples', '64'])
    assert a.tuning_samples == 64 and a.decoder_dtype == 'f32'
    for bad in (['--online', '--online-tuning', '3'], ['--online', '--decoder-dtype', 'bf16'], ['--tuning-samples', '8']):
        with pytest.raises(SystemExit):
            t.parse_args(['cfg.py', 'ck.pth', '--eval', 'iou'] + bad)
