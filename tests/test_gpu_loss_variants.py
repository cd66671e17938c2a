"""GPU parity of the four train_cfg variants of OccBBoxHead.loss_occ (contrastive_loss, residual_loss,
no_loss_for_outside, no_loss_for_observed_feats; each alone and all four together) against the REFERENCE's own head on
the same seeded scene with the same name-hashed weights (tests/golden/ococc_loss_variants.npz,
tools/gen_golden_loss_variants.py), with the model of tests/test_gpu_ococc_train.py and that file's tolerances: rtol 1e-4,
atol 1e-5; the per-sample loss vector atol 2e-4; gradient norms 2e-3.

BAND samples (|ori logit| <= 4e-3 * max |ori logit|, twice the 2e-3 the project grants the decoder's logits, or closer
than 1e-4 m to a face of their box; at most 2 % of the samples, asserted by the generator) are the ones whose ori class
or inside-test may turn on rounding.  The per-sample vector is compared on the other samples.  An entry that is a mean
or a ratio over samples moves by at most one term per flipped sample: it gets n_band / n_counted added to its tolerance,
n_counted the number of samples the reference counted in it (`<setting>/counted_<key>` of the golden; ratios are at most
1, so the share is capped there).  The gradient of the summed loss entries gets the largest share of its entries."""
import os

import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

SWITCHES = ('contrastive_loss', 'residual_loss', 'no_loss_for_outside', 'no_loss_for_observed_feats')
SETTINGS = {'contrastive': ('contrastive_loss',), 'residual': ('residual_loss',), 'outside': ('no_loss_for_outside',),
            'observed': ('no_loss_for_observed_feats',), 'all': SWITCHES}
MASKED = {'contrastive': False, 'residual': True, 'outside': True, 'observed': True, 'all': True}   # a band sample can matter
SAMPLE_MEANS = ('recall_neg', 'recall_pos', 'precision_neg', 'precision_pos', 'loss_rcnn_occ_residual')


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'ococc_loss_variants.npz'), allow_pickle=False)


@pytest.fixture(scope='module')
def model(dev, gold):
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (register)
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    m = DETECTORS.build(ococcnet_model_cfg())
    bh = m.roi_head.bbox_head
    bh.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in bh.state_dict().items()},
                                              seed=int(gold['weight_seed'])))
    return m.to(dev).eval()   # eval: dropout off, as in the generator


def _batch(dev, seed, keep=None):
    from objectcentricocccompletion_amd.tracklet import Tracklet
    samples = synth.synth_training_scene(seed=seed)
    if keep is not None:
        samples = [samples[i] for i in keep]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(points=[T(s['points']) for s in samples], pts_frame_inds=[T(s['pts_frame_inds']) for s in samples],
                img_metas=None, tracklet=[Tracklet(T(s['boxes']), s['ts'], T(s['scores']), type=0) for s in samples],
                gt_tracklet_candidates=[[Tracklet(T(cb), cts, type=0) for (cb, cts, _, _) in s['candidates']] for s in samples],
                occ_labels=[[T(o) for (_, _, o, _) in s['candidates']] for s in samples],
                occ_labels_scores=[[torch.tensor([sc], dtype=torch.float32, device=dev) for (_, _, _, sc) in s['candidates']]
                                   for s in samples])


def _set(model, on, monkeypatch):
    bh = model.roi_head.bbox_head
    for k in SWITCHES:
        monkeypatch.setitem(bh.train_cfg, k, k in on)
    monkeypatch.setattr(bh, 'fused_mode', 'concat_residual' if 'residual_loss' in on else 'concat')


def _forward(model, dev, seed, keep=None):
    torch.manual_seed(123)
    model.zero_grad(set_to_none=True)
    return model(return_loss=True, **_batch(dev, seed, keep))


@pytest.fixture(scope='module')
def kernel_runs():
    return {}   # setting -> the loss dict of the kernel path, for the comparison with OCOCC_OCC_LOSS_KERNEL=0


@pytest.mark.parametrize('setting', list(SETTINGS))
def test_variant_losses_and_gradients_equal_reference(dev, gold, model, setting, monkeypatch, kernel_runs):
    from objectcentricocccompletion_amd import heads
    from objectcentricocccompletion_amd.occ import occ_ops
    assert heads.OCC_LOSS_KERNEL
    calls = []
    real = occ_ops.occ_loss_masks
    monkeypatch.setattr(occ_ops, 'occ_loss_masks', lambda *a, **k: calls.append(1) or real(*a, **k))
    _set(model, SETTINGS[setting], monkeypatch)
    losses = _forward(model, dev, int(gold['seed']))
    assert len(calls) == (1 if MASKED[setting] else 0)             # the masks are ONE call of the kernel's wrapper
    band = gold['band']
    ori, face = gold['ori_logits'], gold['face_dist']
    assert np.array_equal(band, (np.abs(ori) <= 4e-3 * np.abs(ori).max()) | (face <= 1e-4)) and band.mean() <= 0.02
    n_band = int(band.sum()) if MASKED[setting] else 0
    pre = setting + '/loss_'
    counted = lambda k: int(gold[f'{setting}/counted_{k}'])
    share = lambda k: min(1.0, n_band / max(counted(k), 1))
    assert set(losses) == {k[len(pre):] for k in gold.files if k.startswith(pre)} - {'loss_rcnn_occ_residual_mean'}
    for k, v in losses.items():
        got = v.detach().float().cpu().numpy().reshape(-1)
        exp = gold[pre + ('loss_rcnn_occ_residual_mean' if k == 'loss_rcnn_occ_residual' else k)].reshape(-1)
        assert got.shape == exp.shape, k
        print(f'{setting:12s} {k:24s} got {got[:3]} exp {exp[:3]} max|d| {np.abs(got - exp).max():.3e}'
              + (f' share {share(k):.3e}' if k in SAMPLE_MEANS else ''))
    for k, v in losses.items():
        got = v.detach().float().cpu().numpy().reshape(-1)
        exp = gold[pre + ('loss_rcnn_occ_residual_mean' if k == 'loss_rcnn_occ_residual' else k)].reshape(-1)
        if k == 'num_unmatched':
            assert abs(got[0] - exp[0]) <= n_band, (got, exp)
        elif k.startswith('num_'):
            assert np.array_equal(got, exp), k
        elif k == 'loss_rcnn_occ':                    # reduction='none': one BCE term per query point
            keep = ~band if MASKED[setting] else np.ones_like(band)
            assert np.allclose(got[keep], exp[keep], rtol=1e-4, atol=2e-4), (k, np.abs(got - exp)[keep].max())
        elif k in SAMPLE_MEANS:
            assert np.all(np.abs(got - exp) <= 1e-5 + 1e-4 * np.abs(exp) + share(k)), (k, got, exp, share(k))
        else:
            assert np.allclose(got, exp, rtol=1e-4, atol=1e-5), (k, got, exp)
    if 'loss_rcnn_occ_residual' in losses:
        assert losses['loss_rcnn_occ_residual'].dim() == 0 and losses['loss_rcnn_occ_residual'].requires_grad
    kernel_runs[setting] = {k: v.detach().clone() for k, v in losses.items()}
    total = sum(v.mean() for k, v in losses.items() if 'loss' in k)      # tools/train.py, mmdet's _parse_losses
    total.backward()
    params = dict(model.roi_head.bbox_head.named_parameters())
    names, norms = [str(n) for n in gold['grad_names']], gold[f'{setting}/grad_norms']
    assert sorted(names) == sorted(params.keys()) and len(names) == 269
    grad_share = max([share('loss_rcnn_occ')] + ([share('loss_rcnn_occ_residual')] if 'loss_rcnn_occ_residual' in losses else []))
    worst = 0.0
    for n, e in zip(names, norms):
        g = params[n].grad
        got = 0.0 if g is None else float(g.double().norm())
        worst = max(worst, abs(got - e) / max(e, 1e-6 * float(norms.max())))
    print(f'{setting}: worst relative gradient-norm error over {len(names)} parameters: {worst:.2e} (band share {grad_share:.2e})')
    for n, e in zip(names, norms):
        g = params[n].grad
        got = 0.0 if g is None else float(g.double().norm())
        assert abs(got - e) <= (2e-3 + grad_share) * e + 1e-6 * float(norms.max()), (n, got, e)
    model.zero_grad(set_to_none=True)


@pytest.mark.parametrize('setting', ['outside', 'all'])
def test_kernel_and_chain_give_the_same_dict(dev, gold, model, setting, monkeypatch, kernel_runs):
    from objectcentricocccompletion_amd import heads
    from objectcentricocccompletion_amd.occ import occ_ops
    if setting not in kernel_runs:
        _set(model, SETTINGS[setting], monkeypatch)
        kernel_runs[setting] = {k: v.detach().clone() for k, v in _forward(model, dev, int(gold['seed'])).items()}
    monkeypatch.setattr(heads, 'OCC_LOSS_KERNEL', False)            # what OCOCC_OCC_LOSS_KERNEL=0 sets at import
    monkeypatch.setattr(occ_ops, 'occ_loss_masks', None)            # (not callable: the chain form is what runs)
    _set(model, SETTINGS[setting], monkeypatch)
    chain = _forward(model, dev, int(gold['seed']))
    assert set(chain) == set(kernel_runs[setting])
    # (equal masks -- bit for bit, tests/test_gpu_occ_loss_masks.py -- and the same launches behind them; 1e-5 is what
    # two runs of one training step are held to in test_gpu_ococc_train.py, the counts are exact)
    for k, v in chain.items():
        a, b = v.detach().float(), kernel_runs[setting][k].float()
        if k.startswith('num_'):
            assert torch.equal(a, b), k
        else:
            assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-5, atol=1e-6), (k, float((a - b).abs().max()))


def test_residual_loss_needs_a_residual_fused_mode(dev, gold, model, monkeypatch):
    _set(model, ('residual_loss',), monkeypatch)
    monkeypatch.setattr(model.roi_head.bbox_head, 'fused_mode', 'concat')
    with pytest.raises(AssertionError):
        _forward(model, dev, int(gold['seed']))


def test_no_switch_calls_neither_form(dev, gold, model, monkeypatch):
    from objectcentricocccompletion_amd.occ import occ_ops
    monkeypatch.setattr(occ_ops, 'occ_loss_masks', None)
    monkeypatch.setattr(occ_ops, 'occ_loss_masks_aten', None)
    _set(model, (), monkeypatch)
    losses = _forward(model, dev, int(gold['seed']))
    assert not {'loss_contrastive_feats', 'num_unmatched', 'loss_rcnn_occ_residual'} & set(losses)


def test_scene_slice_without_a_positive_roi(dev, gold, model, monkeypatch):
    """tracklet 3 of the scene has no GT candidate: no positive RoI, the zero entries of ococc_bbox_head.py:640-659"""
    _set(model, SWITCHES, monkeypatch)
    losses = _forward(model, dev, int(gold['seed']), keep=[3])
    assert float(losses['num_pos_rois']) == 0
    assert {'loss_contrastive_feats', 'num_unmatched', 'loss_rcnn_occ_residual', 'loss_rcnn_occ'} <= set(losses)
    assert losses['num_unmatched'].shape == (1,) and float(losses['num_unmatched']) == 0
    for k in ('loss_rcnn_occ', 'loss_rcnn_occ_residual'):
        assert losses[k].requires_grad and losses[k].numel() > 0 and not losses[k].detach().any()
    for k in ('recall_neg', 'recall_pos', 'precision_neg', 'precision_pos'):
        assert losses[k].tolist() == [1.0]
    assert float(losses['loss_contrastive_feats'].detach()) > 0 and losses['loss_contrastive_feats'].requires_grad
    sum(v.mean() for k, v in losses.items() if 'loss' in k).backward()          # a live graph with zero gradients behind it
    model.zero_grad(set_to_none=True)


def test_training_mode_step_with_all_switches(dev, gold, model, monkeypatch):
    """the form a user trains with: train() (the decoder's dropout on, also in the ori decode under no_grad, as
    upstream), the decoder's MLP in bf16 (its one-launch training kernels for the two decodes under autograd) -- every
    entry there and finite, the counts in range, gradients behind the two new loss terms"""
    import copy
    from objectcentricocccompletion_amd.occ.occ_base import OccDecoder
    m = copy.deepcopy(model).train()
    for mod in m.modules():
        if isinstance(mod, OccDecoder):
            mod.compute_dtype = torch.bfloat16
    _set(m, SWITCHES, monkeypatch)
    monkeypatch.setitem(m.roi_head.train_cfg, 'random_shift_frame_inds', False)
    losses = _forward(m, dev, int(gold['seed']))
    assert {'loss_contrastive_feats', 'num_unmatched', 'loss_rcnn_occ_residual'} <= set(losses)
    for k, v in losses.items():
        assert bool(torch.isfinite(v.detach()).all()), k
    n = losses['loss_rcnn_occ'].numel()
    assert n == gold['band'].size and 0 < float(losses['num_unmatched']) < n
    for k in ('recall_neg', 'recall_pos', 'precision_neg', 'precision_pos'):
        assert 0.0 <= float(losses[k]) <= 1.0, k
    assert float(losses['loss_rcnn_occ_residual'].detach()) > 0
    (losses['loss_rcnn_occ_residual'] + losses['loss_contrastive_feats']).backward()
    head = m.roi_head.bbox_head
    for p in (head.occ_ae_head.occ_decoder.conv_occ[-1].weight, head.conv_latent[0][0].weight):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
