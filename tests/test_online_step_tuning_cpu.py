"""Tuning per online step, host side (no device): what ``tune=`` reports before anything is launched, the refusals that
stay (test_cfg.online_tuning), the row seeds of (slot, frame) from single and chunked steps, the default from
test_cfg.online_step_tuning, and the flags of the two tools."""
import importlib.util
import os

import pytest
import torch

import tune_sample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNE = dict(num_iter=5, downsample_size=64, balance_sample=True, seed=11)


@pytest.fixture(scope='module', autouse=True)
def _generators_as_found():
    """later tests of the suite initialise networks from torch's global generators without seeding them"""
    cpu = torch.get_rng_state()
    yield
    torch.set_rng_state(cpu)


@pytest.fixture(scope='module')
def model():
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (register)
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    return DETECTORS.build(ococcnet_model_cfg()).eval()


def _frame(n=1):
    return dict(pts_xyz=torch.zeros(4, 3), pts_feats=torch.zeros(4, 7), pts_batch_idx=torch.zeros(4, dtype=torch.long),
                boxes=torch.ones(n, 7), scores=torch.ones(n), labels=torch.zeros(n, dtype=torch.long))


def _tool(name):
    spec = importlib.util.spec_from_file_location('ococc_tools_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tune_on_cpu_tensors_is_reported_as_the_other_steps_report_it(model):
    from objectcentricocccompletion_amd import _lib as L
    rh = model.roi_head
    state = rh.online_begin(3, 'cpu', cap=4)
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        rh.simple_test_step(**_frame(2), slot=[0, 2], state=state, tune=dict(TUNE))
    f = _frame(2)
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        rh.simple_test_steps(f['pts_xyz'], f['pts_feats'], f['pts_batch_idx'], f['boxes'], f['scores'], f['labels'], [1, 1],
                             state, tune=dict(TUNE))
    assert state.frames == [0, 0, 0]
    assert 'online_step_tuning' not in rh.test_cfg and 'online_step_tuning' not in rh.bbox_head.test_cfg   # absent by default


def test_what_tune_cannot_be_is_reported_before_anything_runs(model):
    head = model.roi_head.bbox_head
    cache = model.roi_head.online_begin(2, 'cpu', cap=4).cache
    step = lambda tune: head.forward_step(None, None, None, None, None, None, [0], cache, tune=tune)
    steps = lambda tune: head.forward_steps(None, None, None, None, None, [0, 0], cache, tune=tune)
    for call in (step, steps):
        with pytest.raises(NotImplementedError, match='balance_sample=True with any downsample_size') as e:
            call(dict(num_iter=3, balance_sample=False, downsample_size=64))
        assert 'balance_sample=False with downsample_size=-1' in str(e.value)
        with pytest.raises(ValueError, match='num_iter'):
            call(dict(downsample_size=64))
        with pytest.raises(ValueError, match='tune= takes'):
            call(dict(num_iter=3, samples=64))
        with pytest.raises(ValueError, match='num_iter = -1'):
            call(dict(num_iter=-1))
    assert head._check_tune(None) is None
    assert head._check_tune(dict(num_iter=3)) == (3, -1, True, 0)
    assert head._check_tune(dict(num_iter=3, balance_sample=False)) == (3, -1, False, 0)
    assert head._check_tune(TUNE) == (5, 64, True, 11)
    assert cache.pos_host == [0, 0]


def test_online_tuning_is_still_refused_by_the_steps(model):
    head = model.roi_head.bbox_head
    cache = model.roi_head.online_begin(1, 'cpu', cap=2).cache
    head.test_cfg['online_tuning'] = dict(num_iter=5, downsample_size=64, balance_sample=True)
    try:
        for tune in (None, dict(TUNE)):
            with pytest.raises(NotImplementedError, match='pass `tune=` to the step'):
                head.forward_step(None, None, None, None, None, None, [0], cache, tune=tune)
            with pytest.raises(NotImplementedError, match='test_cfg.online_tuning'):
                head.forward_steps(None, None, None, None, None, [0], cache, tune=tune)
    finally:
        del head.test_cfg['online_tuning']


class _Stubs(object):
    """the head with every device stage stubbed out: what is left is the host logic of the steps -- frame counters,
    the tuner and the seeds it uploads"""

    def __init__(self, head, monkeypatch):
        D = head.roi_feature_channels
        self.seeds, self.kw = [], []
        enc = lambda pts_xyz, pts_features, pts_info, roi_inds, rois: (
            torch.zeros(len(rois), D), torch.ones(len(rois), dtype=torch.bool), torch.zeros(len(rois), D), torch.zeros(4, 3))
        monkeypatch.setattr(head, '_encode_rois', enc)
        monkeypatch.setattr(head, '_pos_embed', lambda frames, boxes: None)

        def bump(x, pos, slots, cache, window):
            for s in slots:
                cache.pos_host[int(s)] += 1
            return x
        monkeypatch.setattr(head.trans_enc, 'step', bump)
        monkeypatch.setattr(head.trans_enc, 'steps', bump)
        monkeypatch.setattr(head, '_fuse_and_predict', lambda local, fused, final, mask, tune=None: dict(
            fused_roi_feats=local if tune is None else tune(local)))

        def step_sample(local_xyz, rois, roi_inds, row_seeds, row_keep, **kw):
            self.seeds.append(row_seeds.tolist())
            self.kw.append(kw)
            z = torch.zeros(0)
            return torch.zeros(0, 3), z.int(), z.int(), z, [0] * len(rois)
        monkeypatch.setattr(head.occ_ae_head, 'step_sample', step_sample)


def test_row_seeds_belong_to_slot_and_frame(model, monkeypatch):
    """row_seeds[j] = mix64(seed ^ (slot_j << 32 | frame_j)): the same from single steps, from single steps in another row
    order and company, and from forward_steps with repeated slots"""
    rh, head = model.roi_head, model.roi_head.bbox_head
    stubs = _Stubs(head, monkeypatch)
    rois = lambda n: torch.zeros(n, 8)
    want = lambda slot, frame: ref.row_seed(TUNE['seed'], slot, frame)
    cache = rh.online_begin(4, 'cpu', cap=8).cache
    for f in range(3):
        head.forward_step(None, None, None, None, rois(2), torch.zeros(2, dtype=torch.long), [0, 2], cache, tune=dict(TUNE))
    assert stubs.seeds == [[want(0, f), want(2, f)] for f in range(3)]
    assert stubs.kw[0] == dict(downsample_size=64, balance_sample=True)
    head.forward_step(None, None, None, None, rois(3), torch.zeros(3, dtype=torch.long), [3, 2, 0], cache, tune=dict(TUNE))
    assert stubs.seeds[-1] == [want(3, 0), want(2, 3), want(0, 3)]
    fresh = rh.online_begin(4, 'cpu', cap=8).cache
    head.forward_steps(None, None, None, None, rois(6), [0, 0, 0, 2, 2, 2], fresh, tune=dict(TUNE))
    assert stubs.seeds[-1] == [want(0, 0), want(0, 1), want(0, 2), want(2, 0), want(2, 1), want(2, 2)]
    head.forward_steps(None, None, None, None, rois(3), [2, 0, 0], fresh, tune=dict(TUNE))
    assert stubs.seeds[-1] == [want(2, 3), want(0, 3), want(0, 4)]
    # another seed of the call: other seeds; no tune: the tuner is never built
    n = len(stubs.seeds)
    head.forward_step(None, None, None, None, rois(1), torch.zeros(1, dtype=torch.long), [1], fresh, tune=dict(TUNE, seed=12))
    assert stubs.seeds[-1] == [ref.row_seed(12, 1, 0)] != [want(1, 0)]
    head.forward_step(None, None, None, None, rois(1), torch.zeros(1, dtype=torch.long), [1], fresh)
    head.forward_step(None, None, None, None, rois(1), torch.zeros(1, dtype=torch.long), [1], fresh, tune=dict(num_iter=0))
    assert len(stubs.seeds) == n + 1


def test_roi_head_passes_tune_and_its_default(model, monkeypatch):
    rh = model.roi_head
    assert rh._step_kwargs(False, None) == {} and rh._step_kwargs(True, None) == {'return_points': True}
    assert rh._step_kwargs(False, TUNE) == {'tune': TUNE}
    monkeypatch.setitem(rh.test_cfg, 'online_step_tuning', dict(num_iter=2))
    assert rh._step_kwargs(True, None) == {'return_points': True, 'tune': dict(num_iter=2)}
    assert rh._step_kwargs(False, TUNE) == {'tune': TUNE}                      # the argument goes first


def test_tool_flags():
    test, raw = _tool('test'), _tool('online_raw')
    base = ['cfg.py', 'ck.pth', '--eval', 'iou']
    a = test.parse_args(base + ['--online', '--step-tuning', '3', '--step-tuning-samples', '64'])
    assert a.step_tuning == 3 and a.step_tuning_samples == 64 and a.online
    assert test.parse_args(base + ['--online']).step_tuning is None
    for bad in (['--step-tuning', '3'], ['--online', '--step-tuning', '-1'], ['--online', '--step-tuning-samples', '64'],
                ['--online', '--online-tuning', '3']):
        with pytest.raises(SystemExit):
            test.parse_args(base + bad)
    rbase = ['cfg.py', 'ck.pth', 'raw.yaml']
    a = raw.parse_args(rbase + ['--step-tuning', '2'])
    assert a.step_tuning == 2 and a.step_tuning_samples is None
    assert raw.parse_args(rbase).step_tuning is None
    for bad in (['--step-tuning', '-1'], ['--step-tuning-samples', '64']):
        with pytest.raises(SystemExit):
            raw.parse_args(rbase + bad)
