"""Online inference, host side (no device): the bookkeeping of the temporal K/V cache and everything the step path
reports before it launches anything -- a step past the cache, duplicate slots, CPU tensors, training mode, the two test_cfg
switches that cannot run frame by frame -- and the new export's declaration, symbol, binding and INTEGRATION.md row."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'ococc_temporal_attention_step_f32'


@pytest.fixture(scope='module', autouse=True)
def _generators_as_found():
    """later tests of the suite initialise networks from torch's global generators without seeding them: leave both
    as this module found them"""
    cpu = torch.get_rng_state()
    gpu = torch.cuda.get_rng_state() if torch.cuda.is_available() else None
    yield
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state(gpu)


@pytest.fixture(scope='module')
def model():
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (register)
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    return DETECTORS.build(ococcnet_model_cfg()).eval()


def _frame(n=1):
    """one frame of n tracklets as simple_test_step takes it, on the host"""
    return dict(pts_xyz=torch.zeros(4, 3), pts_feats=torch.zeros(4, 7), pts_batch_idx=torch.zeros(4, dtype=torch.long),
                boxes=torch.ones(n, 7), scores=torch.ones(n), labels=torch.zeros(n, dtype=torch.long))


def test_cache_bookkeeping():
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ.layers import TemporalCache
    c = TemporalCache(3, 4, 64, 'cpu', cap=2)
    assert len(c.k) == len(c.v) == 3 and c.k[0].shape == (4, 2, 64) and c.k[0].dtype == torch.float32
    assert c.pos.dtype == torch.int32 and c.pos.tolist() == c.pos_host == [0, 0, 0, 0]
    assert c.nbytes() == 2 * 3 * 4 * 2 * 64 * 4
    assert TemporalCache(3, 1, 1536, 'cpu', cap=1).nbytes() * 256 == 9437184          # the ococcnet model: 9.4 MB per slot
    assert c.check_step([3, 1]) == [3, 1]
    slot = torch.tensor([3, 1], dtype=torch.int32)
    c.advance([3, 1], slot)
    c.advance([3], slot[:1])
    assert c.pos_host == [0, 1, 0, 2] and c.pos.tolist() == [0, 1, 0, 2]
    with pytest.raises(L.OcoccError, match='cap = 2'):
        c.check_step([1, 3])                                                         # slot 3 is full
    with pytest.raises(L.OcoccError, match='duplicate'):
        c.check_step([1, 1])
    with pytest.raises(L.OcoccError, match='outside'):
        c.check_step([4])
    c.reset([3])
    assert c.pos_host == [0, 1, 0, 0] and c.pos.tolist() == [0, 1, 0, 0] and c.check_step([3]) == [3]
    c.reset()
    assert c.pos_host == [0, 0, 0, 0] and c.pos.tolist() == [0, 0, 0, 0]
    with pytest.raises(L.OcoccError):
        TemporalCache(3, 1, 64, 'cpu', cap=257)


@pytest.mark.parametrize('kind', ['plain', 'ring', 'long'])
def test_check_step_is_check_steps_over_distinct_slots(kind):
    """check_step(s) is check_steps(s) for runs of one frame plus the refusal of duplicates: on every list of distinct
    slots of a 4-slot cache (slots at 0 frames, in mid-tracklet, one below the limit, at the limit) both return the same
    rows, with offsets 0 and runs of 1, or both raise OcoccError; [1, 1] is a run of two to check_steps and a duplicate
    to check_step; neither touches pos_host"""
    import itertools
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ.layers import TemporalCache
    c = TemporalCache(1, 4, 8, 'cpu', **dict(plain=dict(cap=2), ring=dict(cap=3, ring=True), long=dict(cap=300, long=True))[kind])
    limit = c.MAX_FRAMES if c.ring else c.cap
    c.pos_host = [0, 0, limit - 1, limit]                                           # slot 3 is full / its counter is spent
    before = list(c.pos_host)

    def outcome(check, slots):
        try:
            return check(slots)
        except L.OcoccError as e:
            return str(e)

    lists = [list(p) for n in range(5) for p in itertools.permutations(range(4), n)] + [[4], [0, 4], [-1], [2, 5, 1]]
    raised = 0
    for slots in lists:
        one, many = outcome(c.check_step, slots), outcome(c.check_steps, slots)
        if isinstance(many, str):                                                    # the same refusal, word for word
            assert one == many and (3 in slots or min(slots) < 0 or max(slots) > 3), slots
            raised += 1
        else:
            assert one == many[0] == slots and many[1] == [0] * len(slots) and many[2] == {s: 1 for s in slots}, slots
    assert raised == len([s for s in lists if 3 in s or min(s, default=0) < 0 or max(s, default=0) > 3]) > 0
    for check in (c.check_step, c.check_steps):
        with pytest.raises(L.OcoccError, match='outside 0..3'):
            check([0, 4])
        with pytest.raises(L.OcoccError, match=re.escape('2**31') if c.ring else f'cap = {c.cap}'):
            check([3])
    if not c.ring:
        with pytest.raises(L.OcoccError, match='<= 4096' if kind == 'long' else '<= 256'):
            c.check_step([3])
    with pytest.raises(L.OcoccError, match='duplicate'):
        c.check_step([1, 1])
    assert c.check_steps([1, 1]) == ([1, 1], [0, 1], {1: 2})
    assert c.pos_host == before and c.pos.tolist() == [0, 0, 0, 0]


def test_encoder_step_reports_on_the_host():
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ.layers import SimpleEncoderLayer, TemporalCache, TransformerEncoder
    enc = TransformerEncoder(SimpleEncoderLayer(64, 4, dim_feedforward=32), 3).eval()
    c = TemporalCache(3, 2, 64, 'cpu', cap=1)
    x = torch.zeros(2, 64)
    with pytest.raises(L.OcoccError, match='duplicate'):
        enc.step(x, x, [0, 0], c)
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        enc.step(x, x, [0, 1], c)
    c.pos_host[1] = 1
    with pytest.raises(L.OcoccError, match='cap = 1'):
        enc.step(x, x, [0, 1], c)
    with pytest.raises(L.OcoccError, match='layers'):
        enc.step(x, x, [0], TemporalCache(2, 2, 64, 'cpu', cap=1))
    assert c.pos_host == [0, 1]                                                      # nothing advanced
    layer, att = enc.layers[0], enc.layers[0].self_attn
    slot, pos = torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        att.step(x, x, slot, c.k[0], c.v[0], pos)
    enc.train()
    for call in (lambda: enc.step(x, x, [0, 1], c), lambda: layer.step(x, x, slot, c.k[0], c.v[0], pos),
                 lambda: att.step(x, x, slot, c.k[0], c.v[0], pos)):
        with pytest.raises(RuntimeError, match='inference only'):
            call()


def test_roi_head_step_reports_on_the_host(model):
    from objectcentricocccompletion_amd import _lib as L
    rh = model.roi_head
    state = rh.online_begin(3, 'cpu', cap=2)
    assert state.slots == 3 and state.frames == [0, 0, 0] and state.cache.cap == 2
    assert state.cache.num_layers == 3 and state.cache.embed_dim == 1536
    assert rh.online_begin(1, 'cpu').cache.cap == 256
    with pytest.raises(L.OcoccError, match='duplicate'):
        rh.simple_test_step(**_frame(2), slot=[1, 1], state=state)
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        rh.simple_test_step(**_frame(2), slot=[0, 2], state=state)
    state.cache.pos_host[2] = 2
    with pytest.raises(L.OcoccError, match='cap = 2'):
        rh.simple_test_step(**_frame(2), slot=[0, 2], state=state)
    state.reset([2])
    assert state.frames == [0, 0, 0]
    model.train()
    try:
        with pytest.raises(RuntimeError, match='inference only'):
            rh.simple_test_step(**_frame(1), slot=[0], state=state)
        with pytest.raises(RuntimeError, match='inference only'):
            rh.bbox_head.forward_step(None, None, None, None, None, None, [0], state.cache)
    finally:
        model.eval()


def test_switches_that_cannot_run_frame_by_frame(model):
    rh, head = model.roi_head, model.roi_head.bbox_head
    state = rh.online_begin(1, 'cpu', cap=1)
    args = (None, None, None, None, None, None, [0], state.cache)
    for key, exc in (('allow_attn_future', ValueError), ('online_tuning', NotImplementedError)):
        head.test_cfg[key] = True
        try:
            with pytest.raises(exc):
                head.forward_step(*args)
        finally:
            del head.test_cfg[key]
    assert not rh.test_cfg.get('online', False)                                      # the new key: off unless asked for
    rh.test_cfg['online'] = True
    try:
        with pytest.raises(NotImplementedError):
            model.aug_test([[None]], [[None]], [[None]], [[None]])
        with pytest.raises(Exception) as e:                                          # simple_test goes the online way
            rh.simple_test(torch.zeros(1, 3), torch.zeros(1, 7), torch.zeros(1, dtype=torch.long),
                           torch.zeros(1, dtype=torch.long), None, [_one_frame_tracklet()])
        assert 'CPU tensor' in str(e.value)
    finally:
        rh.test_cfg['online'] = False
    assert state.frames == [0]


def _one_frame_tracklet():
    from objectcentricocccompletion_amd.tracklet import Tracklet
    return Tracklet(torch.ones(1, 7), [0], torch.ones(1), type=0)


def test_export_is_declared_bound_and_documented():
    import ctypes
    from objectcentricocccompletion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ococc_hip.h')).read()
    m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % NAME, re.sub(r'/\*.*?\*/', '', header, flags=re.S))
    assert m, f'{NAME} is not declared in ococc_hip.h'
    assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[NAME][1]) == 20
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME) and hasattr(_lib.lib, NAME)
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert any(f'`{NAME}`' in line and line.startswith('|') for line in integration.splitlines()), 'no INTEGRATION.md row'
    src = open(os.path.join(ROOT, 'objectcentricocccompletion_amd', 'csrc', 'Makefile')).read()
    assert 'causal_attn_step.hip' in src
    # invalid arguments are reported, not thrown, before anything is dereferenced or launched
    bad = lambda cap, D: _lib.lib.ococc_temporal_attention_step_f32(None, 0, None, 0, None, 0, None, None, None, None, 1, 1, cap,
                                                                    1, D, 1.0, 0, None, 0, None)
    assert bad(257, 8) == -1 and b'256' in _lib.lib.ococc_last_error()
    assert bad(8, 6) == -1 and bad(8, 388) == -1
    assert bad(8, 8) == -1 and b'null pointer' in _lib.lib.ococc_last_error()


def test_tool_flag_and_first_frame_pose():
    """tools/test.py --online: the flag, and the pipeline's TrackletPoseTransform switched to the first frame's ego pose
    (the one frame an online caller knows); the transform with shared_frame='first' leaves frame 0 where it is"""
    import importlib.util
    from objectcentricocccompletion_amd import pipelines as P
    from objectcentricocccompletion_amd.tracklet import Tracklet
    spec = importlib.util.spec_from_file_location('ococc_tools_test', os.path.join(ROOT, 'tools', 'test.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert not tool.parse_args(['cfg.py', 'ck.pth', '--eval', 'iou']).online
    args = tool.parse_args(['cfg.py', 'ck.pth', '--eval', 'iou', '--online'])
    assert args.online
    steps = {s['type']: s for s in tool.build_test_dataset_cfg({}, args)['pipeline']}
    assert steps['TrackletPoseTransform']['shared_frame'] == 'first' and 'shared_frame' not in steps['PointDecoration']
    args.online = False
    assert all('shared_frame' not in s for s in tool.build_test_dataset_cfg({}, args)['pipeline'])
    g = torch.Generator().manual_seed(0)
    L = 5
    poses = []
    for i in range(L):   # ego -> world: a yaw and a translation per frame
        a = 0.1 * i
        m = torch.eye(4)
        m[:2, :2] = torch.tensor([[torch.cos(torch.tensor(a)), -torch.sin(torch.tensor(a))],
                                  [torch.sin(torch.tensor(a)), torch.cos(torch.tensor(a))]])
        m[:3, 3] = torch.tensor([2.0 * i, 0.5 * i, 0.0])
        poses.append(m)
    pts = [torch.randn(6, 5, generator=g) for _ in range(L)]
    boxes = torch.cat([torch.randn(L, 3, generator=g), torch.rand(L, 3, generator=g) + 1, torch.randn(L, 1, generator=g)], 1)

    def run(shared_frame):
        trk = Tracklet(boxes.clone(), list(range(L)))
        trk.pose_list = list(poses)
        d = dict(points=[p.clone() for p in pts], tracklet=trk, pts_frame_inds=[torch.full((6,), i) for i in range(L)])
        P.TrackletPoseTransform(concat=False, shared_frame=shared_frame)(d)
        return d
    first, mid = run('first'), run('middle')
    assert torch.equal(first['shared_pose'], poses[0]) and torch.equal(mid['shared_pose'], poses[L // 2])
    assert torch.allclose(first['points'][0], pts[0], atol=1e-5) and torch.allclose(mid['points'][L // 2], pts[L // 2], atol=1e-5)
    assert torch.allclose(first['tracklet'].boxes[0], boxes[0], atol=1e-5)
    assert not torch.allclose(first['points'][L // 2][:, :3], pts[L // 2][:, :3], atol=1e-3)
    with pytest.raises(AssertionError):
        P.TrackletPoseTransform(shared_frame='last')
