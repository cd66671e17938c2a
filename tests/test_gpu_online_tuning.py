"""test_cfg.online_tuning in the full head (OccBBoxHead.forward, ococc_bbox_head.py:371-431) on the MI355X: the fused
shape latent of every RoI tuned against the RoI's own observation, on the kernels of occ/latent_tune.py (bf16 decoder) and
through autograd (OCOCC_LATENT_TUNE_KERNELS=0, f32 decoder), and tools/test.py --online-tuning end to end."""
import ast
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'ococcnet_mi355x.py')
TUNING = dict(num_iter=5, downsample_size=64, balance_sample=True)
PICK = [0, 1, 2, 32, 33, 34]     # RoIs of tests/golden/ococc_head.npz: 2 tracklets x 3 frames; RoI 0 holds no point
EMPTY = 0


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


@pytest.fixture(scope='module')
def head(dev):
    """The reference-sized head as tests/test_gpu_ococc.py builds it, with the bf16 decoder."""
    from objectcentricocccompletion_amd import heads  # noqa: F401
    from objectcentricocccompletion_amd.occ.occ_base import OccDecoder
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import HEADS
    cfg = ococcnet_model_cfg()
    hc = dict(cfg['roi_head']['bbox_head'])
    hc['train_cfg'], hc['test_cfg'] = cfg['train_cfg'], dict(cfg['test_cfg'])
    h = HEADS.build(hc)
    h.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in h.state_dict().items()}, seed=0))
    h = h.to(dev).eval()
    for m in h.modules():
        if isinstance(m, OccDecoder):
            m.compute_dtype = torch.bfloat16
    return h


@pytest.fixture(scope='module')
def inputs(dev, golden_dir):
    gold = np.load(os.path.join(golden_dir, 'ococc_head.npz'))
    T = lambda k: torch.from_numpy(gold['in_' + k])
    roi_inds = T('roi_inds')
    new = torch.full((64,), -1, dtype=torch.long)
    new[PICK] = torch.arange(len(PICK))
    sel = new[roi_inds] >= 0
    rois = T('rois')[PICK].clone()
    frames = torch.tensor([0, 1, 2, 0, 1, 2])
    counts = torch.bincount(new[roi_inds][sel], minlength=len(PICK))
    assert counts[EMPTY] == 0 and bool((counts[1:] > 0).all())
    info = dict(local_xyz=T('local_xyz')[sel].to(dev), boundary_offset=T('boundary_offset')[sel].to(dev),
                is_in_margin=T('is_in_margin')[sel].to(dev))
    return (T('pts_xyz')[sel].to(dev), T('pts_feats')[sel].to(dev), info, new[roi_inds][sel].to(dev), rois.to(dev),
            frames.to(dev))


def _forward(head, inputs, tuning, seed=0):
    head.test_cfg.pop('online_tuning', None)
    if tuning is not None:
        head.test_cfg['online_tuning'] = dict(tuning)
    try:
        torch.manual_seed(seed)
        with torch.no_grad():
            out = head(*inputs)
        torch.cuda.synchronize()
        return out
    finally:
        head.test_cfg.pop('online_tuning', None)


@pytest.fixture(scope='module')
def plain(head, inputs):
    return _forward(head, inputs, None)


def test_forward_tunes_the_fused_latent(dev, head, inputs, plain, monkeypatch):
    """The key was accepted and ignored before: fused_roi_feats, cls_score and bbox_pred see the tuned latent,
    ori_roi_feats does not, the RoI without points keeps its latent bit for bit.  (The point encoders sum with float
    atomics: two forward passes agree to rounding, not in every bit -- so what tuning was given and what it handed back
    are taken from inside the one tuned pass, and the pass without the key is compared to rounding.)"""
    from objectcentricocccompletion_amd.occ import latent_tune
    assert latent_tune.supported(head.occ_ae_head.occ_decoder, plain['fused_roi_feats'])
    seen = {}
    real_tune, real_encode = head.online_tuning, head.occ_ae_head.encode

    def tune(latent, *a, **k):
        seen['in'], seen['kw'] = latent, k
        seen['out'] = real_tune(latent, *a, **k)
        return seen['out']

    def encode(*a, **k):
        seen['local'] = real_encode(*a, **k)
        return seen['local']
    monkeypatch.setattr(head, 'online_tuning', tune)
    monkeypatch.setattr(head.occ_ae_head, 'encode', encode)
    hook = head.conv_fused.register_forward_hook(lambda m, i, o: seen.update(fused_in=i[0], fused_out=o))
    try:
        tuned = _forward(head, inputs, TUNING)
    finally:
        hook.remove()
    assert seen['kw'] == dict(downsample_size=64, balance_sample=True, num_iter=5)
    a, b = seen['in'], tuned['fused_roi_feats']
    assert b is seen['out'] and a.shape == b.shape and b.dtype == a.dtype and not b.requires_grad
    live = torch.arange(len(PICK), device=dev) != EMPTY
    moved = (a - b).abs().amax(1)
    print('largest move of the latent per RoI:', [f'{v:.4f}' for v in moved.tolist()])
    assert bool((moved[live] > 0).all()) and torch.equal(a[EMPTY], b[EMPTY])
    # against the pass without the key: what tuning was given is that pass's latent (to rounding), what it handed back is not
    scale = float(plain['fused_roi_feats'].abs().max())
    noise = float((a - plain['fused_roi_feats']).abs().max())
    away = (b - plain['fused_roi_feats']).abs().amax(1)
    print(f'two passes differ by {noise:.2e} of {scale:.2f}; tuned - untuned per RoI {[f"{v:.4f}" for v in away.tolist()]}')
    assert noise <= 1e-4 * scale and bool((away[live] >= 0.009).all()) and float(away[EMPTY]) <= 1e-4 * scale
    assert torch.equal(tuned['ori_roi_feats'], seen['local'][0])                 # the encoder's latent, untouched
    assert float((tuned['ori_roi_feats'] - plain['ori_roi_feats']).abs().max()) <= 1e-4 * float(plain['ori_roi_feats'].abs().max())
    assert torch.equal(plain['nonempty_roi_mask'], tuned['nonempty_roi_mask'])
    # the heads read the tuned latent: conv_fused was given it, the scores are recomputed from what came back
    Dl = head.roi_feature_channels
    assert torch.equal(seen['fused_in'][:, :Dl], b)
    with torch.no_grad():
        fused = head.conv_fused(torch.cat([b, seen['fused_in'][:, Dl:]], dim=1))
        assert torch.equal(head.conv_cls(fused), tuned['cls_score']) and torch.equal(head.conv_reg(fused), tuned['bbox_pred'])


def _observation_loss(head, latent, local_xyz, rois, roi_inds, seed):
    """mean BCE of the decoder per RoI at the cells sampled under ``seed`` (the sample online_tuning draws under it)"""
    torch.manual_seed(seed)
    ae = head.occ_ae_head
    xyz, labels, inds = ae.sample_observation(local_xyz, rois, roi_inds, downsample_size=TUNING['downsample_size'],
                                              balance_sample=True)
    with torch.no_grad():
        logits = ae.decode(latent, xyz, inds).view(-1).double()
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels.double(), reduction='none')
    R = latent.size(0)
    tot = torch.zeros(R, dtype=torch.float64, device=latent.device).index_add_(0, inds.long(), loss)
    cnt = torch.bincount(inds.long(), minlength=R)
    return tot / cnt.clamp(min=1), float(loss.mean())


def _tune(head, latent, local_xyz, rois, roi_inds, seed, kernels, monkeypatch, num_iter=TUNING['num_iter']):
    from objectcentricocccompletion_amd.occ import latent_tune
    monkeypatch.setattr(latent_tune, 'KERNELS', kernels)
    torch.manual_seed(seed)
    with torch.no_grad():
        out = head.online_tuning(latent, local_xyz, rois, roi_inds, downsample_size=TUNING['downsample_size'],
                                 balance_sample=True, num_iter=num_iter)
    torch.cuda.synchronize()
    return out


def test_observation_loss_falls_on_both_paths(dev, head, inputs, plain, monkeypatch):
    """The loss tuning minimises, evaluated outside the loop at the cells of the same seed, before tuning and after 1..5
    iterations: it falls for every RoI with points, and the fall on the kernels is within 10 % of the fall through
    autograd (both run the same bf16 decoder; they differ where Adam's first steps amplify rounding)."""
    seed = 7
    latent = plain['fused_roi_feats']
    with torch.no_grad():
        local_xyz = head._encode_rois(*inputs[:5])[3]
    rois, roi_inds = inputs[4], inputs[3]
    live = torch.arange(len(PICK), device=dev) != EMPTY
    before, before_all = _observation_loss(head, latent, local_xyz, rois, roi_inds, seed)
    curves = {}
    for kernels in (True, False):
        curve = [before_all]
        for n in range(1, TUNING['num_iter'] + 1):
            tuned = _tune(head, latent, local_xyz, rois, roi_inds, seed, kernels, monkeypatch, n)
            per_roi, total = _observation_loss(head, tuned, local_xyz, rois, roi_inds, seed)
            curve.append(total)
        curves[kernels] = curve
        print(('kernels ' if kernels else 'autograd') + ' loss after 0..5 iterations: ' + ' '.join(f'{v:.5f}' for v in curve))
        print('   per RoI before ' + ' '.join(f'{v:.4f}' for v in before.tolist()) + '  after ' + ' '.join(f'{v:.4f}' for v in per_roi.tolist()))
        assert bool((per_roi[live] < before[live]).all()), (kernels, before.tolist(), per_roi.tolist())
        assert torch.equal(tuned[EMPTY], latent[EMPTY])
        assert curve[-1] < curve[0], curve
    fall_k, fall_a = curves[True][0] - curves[True][-1], curves[False][0] - curves[False][-1]
    assert fall_a > 0 and abs(fall_k - fall_a) <= 0.1 * fall_a, (fall_k, fall_a)


def test_train_mode_and_single_steps(dev, head, inputs, monkeypatch):
    """train() mode does not tune; forward_step keeps refusing the key."""
    tuned = []
    real = head.online_tuning
    monkeypatch.setattr(head, 'online_tuning', lambda *a, **k: (tuned.append(1), real(*a, **k))[1])
    head.test_cfg['online_tuning'] = dict(TUNING)
    try:
        head.train()
        with torch.no_grad():
            out = head(*inputs)
        assert not tuned and out['fused_roi_feats'].shape[0] == len(PICK)
        head.eval()
        with torch.no_grad():
            head(*inputs)
        assert tuned                                                  # (the same call in eval mode does)
        with pytest.raises(NotImplementedError):
            head.forward_step(*inputs, [0] * len(PICK), None)
    finally:
        head.test_cfg.pop('online_tuning', None)
        head.eval()


def test_f32_decoder_takes_the_fallback(dev, head, inputs, plain, monkeypatch):
    from objectcentricocccompletion_amd.occ import latent_tune
    dec = head.occ_ae_head.occ_decoder
    monkeypatch.setattr(dec, 'compute_dtype', None)
    assert not latent_tune.supported(dec, plain['fused_roi_feats'])
    called = []
    real = head.occ_ae_head.online_tuning_forward
    monkeypatch.setattr(head.occ_ae_head, 'online_tuning_forward', lambda *a, **k: (called.append(1), real(*a, **k))[1])
    seed = 7
    with torch.no_grad():
        local_xyz = head._encode_rois(*inputs[:5])[3]
    latent = plain['fused_roi_feats']
    live = torch.arange(len(PICK), device=dev) != EMPTY
    before, before_all = _observation_loss(head, latent, local_xyz, inputs[4], inputs[3], seed)
    tuned = _tune(head, latent, local_xyz, inputs[4], inputs[3], seed, True, monkeypatch)
    after, after_all = _observation_loss(head, tuned, local_xyz, inputs[4], inputs[3], seed)
    print(f'f32 decoder (autograd): loss {before_all:.5f} -> {after_all:.5f}')
    assert called and not tuned.requires_grad
    assert bool((after[live] < before[live]).all()) and after_all < before_all and torch.equal(tuned[EMPTY], latent[EMPTY])
    assert not any(p.requires_grad for p in head.occ_ae_head.parameters()) and not head.occ_ae_head.training


def _run(cmd, timeout=600):
    p = subprocess.Popen(cmd, cwd=ROOT, env=dict(os.environ), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out, err = p.communicate(timeout=timeout)
    assert p.returncode == 0, out[-2000:] + err[-3000:]
    return out


def test_tools_test_online_tuning(dev, tmp_path):
    """tools/test.py --online-tuning 3 --decoder-dtype bf16 --eval iou on the synthetic dataset: other IoU counts than
    without the flag."""
    from objectcentricocccompletion_amd import config, heads, point_pool, roi_head  # noqa: F401
    from objectcentricocccompletion_amd.registry import DETECTORS
    data, ckpt = str(tmp_path / 'data'), str(tmp_path / 'ck.pth')
    _run([sys.executable, 'tools/make_synthetic_dataset.py', data, '--tracklets', '2', '--frames', '40'], timeout=300)
    torch.manual_seed(0)
    torch.save({'state_dict': DETECTORS.build(config.fromfile(CFG)['model']).state_dict()}, ckpt)
    res = []
    for extra in ([], ['--online-tuning', '3']):
        out_pkl = str(tmp_path / f'r{len(extra)}.pkl')
        stdout = _run(['timeout', '-k', '10', '540', sys.executable, 'tools/test.py', CFG, ckpt, '--data-root', data, '--eval', 'iou',
                       '--decoder-dtype', 'bf16', '--out', out_pkl] + extra)
        metrics = ast.literal_eval([l for l in stdout.strip().splitlines() if l.startswith('{')][-1])
        with open(out_pkl, 'rb') as f:
            r = pickle.load(f)
        res.append((metrics, torch.cat([torch.cat(x['inters']) for x in r]), torch.cat([torch.cat(x['unions']) for x in r])))
    (m0, i0, u0), (m1, i1, u1) = res
    print('iou without / with tuning:', m0.get('iou'), m1.get('iou'))
    assert i0.numel() > 0 and i1.numel() > 0 and bool((i1 <= u1).all())
    assert not (torch.equal(i0, i1) and torch.equal(u0, u1))
