"""Several frames per tracklet in one online step, host side (no device): the chunk export of the attention step
(csrc/causal_attn_step.hip, ococc_temporal_attention_chunk_f32) is declared, bound and documented and reports argument
errors before it dereferences or launches anything; the bookkeeping of TemporalCache.check_steps / advance; ``steps``
on CPU tensors; test_cfg.online_chunk and tools/test.py --online-chunk."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'ococc_temporal_attention_chunk_f32'


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


def test_export_is_declared_bound_and_documented():
    from objectcentricocccompletion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ococc_hip.h')).read()
    m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % NAME, re.sub(r'/\*.*?\*/', '', header, flags=re.S))
    assert m, f'{NAME} is not declared in ococc_hip.h'
    args = [' '.join(a.split()) for a in m.group(1).split(',')]
    assert len(args) == len(_lib.SIGNATURES[NAME][1]) == 22
    long = _lib.SIGNATURES['ococc_temporal_attention_step_long_f32'][1]
    assert _lib.SIGNATURES[NAME][1] == long[:7] + [ctypes.c_void_p] + long[7:]      # ``off`` after ``slot``
    assert args[6] == 'const int32_t* slot' and args[7] == 'const int32_t* off' and args[8] == 'const int32_t* pos'
    assert args[17] == 'int32_t window' and args[18] == 'int32_t ring'
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME) and hasattr(_lib.lib, NAME)
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert any(f'`{NAME}`' in line and line.startswith('|') for line in integration.splitlines()), 'no INTEGRATION.md row'
    declared = set(re.findall(r'\b(ococc_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S)))
    assert declared == set(_lib.SIGNATURES)


def _call(cap=8, D=8, window=0, ring=0, n=1, slots=1, ptr=None):
    from objectcentricocccompletion_amd import _lib
    return _lib.lib.ococc_temporal_attention_chunk_f32(ptr, 8, ptr, 8, ptr, 8, ptr, ptr, ptr, ptr, ptr, n, slots, cap, 1, D, 1.0,
                                                       window, ring, ptr, 8, None)


def test_argument_errors_are_reported_before_anything_is_touched():
    """every call passes null pointers: a check that ran after a dereference or a launch would not return"""
    from objectcentricocccompletion_amd import _lib
    err = _lib.lib.ococc_last_error
    assert _call(D=6) == -1 and b'multiple of 4' in err()
    assert _call(D=388) == -1 and b'384' in err()
    assert _call(cap=4097) == -1 and b'4096' in err()
    for window in (0, -1, 9):
        assert _call(cap=8, window=window, ring=1) == -1 and b'ring' in err(), window
    assert _call(cap=4097, window=3, ring=1) == -1 and b'4096' in err()
    # valid sizes -- more rows than slots among them, a slot may have several: the pointers are what is wrong
    for kw in (dict(), dict(n=5, slots=1), dict(cap=4096), dict(cap=8, window=8, ring=1), dict(cap=8, window=1, ring=1),
               dict(cap=300, window=3)):
        assert _call(**kw) == -1 and b'null pointer' in err(), kw
    with pytest.raises(_lib.OcoccError):
        _lib.check(_call(), 'temporal_attention_chunk')
    assert _call(n=0) == 0                                                   # an empty call is no error


def test_check_steps_bookkeeping():
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ.layers import TemporalCache
    c = TemporalCache(2, 6, 8, 'cpu', cap=8)
    c.pos_host[:] = [7, 0, 0, 5, 0, 6]
    c.pos.copy_(torch.tensor(c.pos_host, dtype=torch.int32))
    slots, offsets, runs = c.check_steps([3, 3, 3, 0, 5, 5])
    assert slots == [3, 3, 3, 0, 5, 5] and offsets == [0, 1, 2, 0, 0, 1] and runs == {3: 3, 0: 1, 5: 2}
    assert list(runs) == [3, 0, 5]                                           # in order of appearance
    assert c.check_steps(torch.tensor([1, 1]).tolist()) == ([1, 1], [0, 1], {1: 2})
    assert c.check_steps([]) == ([], [], {})
    assert c.check_steps([1] * 8)[2] == {1: 8}                               # room for the whole run: exactly cap
    state = (list(c.pos_host), c.pos.clone())
    for rows, match in (([0, 1, 0], 'not consecutive'), ([3, 3, 0, 3], 'not consecutive'), ([6], 'outside 0..5'),
                        ([1, -1], 'outside 0..5'), ([1] * 9, 'cap = 8'), ([3, 3, 3, 3], 'cap = 8'), ([5, 5, 0, 0], 'cap = 8')):
        with pytest.raises(L.OcoccError, match=match):
            c.check_steps(rows)
        assert c.pos_host == state[0] and torch.equal(c.pos, state[1])       # nothing is modified when it raises
    slot_dev = torch.tensor(slots, dtype=torch.int32)
    c.advance(slots, slot_dev)
    assert c.pos_host == [8, 0, 0, 8, 0, 8] and c.pos.tolist() == c.pos_host
    with pytest.raises(L.OcoccError, match='cap = 8'):
        c.check_steps([2, 0])
    with pytest.raises(L.OcoccError, match='duplicate'):                     # the single-frame check is as it was
        c.check_step([1, 1])

    ring = TemporalCache(1, 2, 8, 'cpu', cap=3, ring=True)
    assert ring.check_steps([1] * 7 + [0] * 4)[2] == {1: 7, 0: 4}            # a ring takes runs longer than cap
    ring.pos_host[1] = 2 ** 31 - 1 - 7
    assert ring.check_steps([1] * 7)[1] == list(range(7))                    # up to the last frame the counter holds
    with pytest.raises(L.OcoccError, match='2\\*\\*31'):
        ring.check_steps([1] * 8)
    ring.pos_host[1] = 2 ** 31 - 1
    with pytest.raises(L.OcoccError, match='2\\*\\*31'):
        ring.check_steps([0, 1])
    assert ring.pos_host == [0, 2 ** 31 - 1] and ring.pos.tolist() == [0, 0]
    long = TemporalCache(1, 1, 8, 'cpu', cap=300, long=True)
    long.pos_host[0] = 290
    assert long.check_steps([0] * 10)[2] == {0: 10}
    with pytest.raises(L.OcoccError, match='cap = 300'):
        long.check_steps([0] * 11)


def test_steps_on_cpu_tensors_raise_after_the_ring_window_check():
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ.layers import SimpleEncoderLayer, TemporalCache, TransformerEncoder
    enc = TransformerEncoder(SimpleEncoderLayer(64, 4, dim_feedforward=32), 3).eval()
    c = TemporalCache(3, 2, 64, 'cpu', cap=3, ring=True)
    x = torch.zeros(5, 64)
    rows = [1, 1, 1, 1, 0]                                                   # a run longer than the ring
    for window in (-1, 0, 4):
        with pytest.raises(L.OcoccError, match='ring'):
            enc.steps(x, x, rows, c, window)
    with pytest.raises(L.OcoccError, match='ring'):
        enc.steps(x, x, rows, c)                                             # (the default window is -1)
    for window in (1, 3):
        with pytest.raises(L.OcoccError, match='CPU tensor'):
            enc.steps(x, x, rows, c, window)
        with pytest.raises(L.OcoccError, match='CPU tensor'):
            enc.steps(x, x, torch.tensor(rows), c, window)
    with pytest.raises(L.OcoccError, match='not consecutive'):
        enc.steps(x, x, [1, 0, 1, 1, 1], c, 3)
    with pytest.raises(L.OcoccError, match='4 slots for 5 rows'):
        enc.steps(x, x, rows[:4], c, 3)
    assert c.pos_host == [0, 0] and c.pos.tolist() == [0, 0]
    plain = TemporalCache(3, 2, 64, 'cpu', cap=4)
    with pytest.raises(L.OcoccError, match='cap = 4'):
        enc.steps(x, x, [0] * 5, plain)
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        enc.steps(x, x, [0, 0, 0, 0, 1], plain)
    with pytest.raises(L.OcoccError, match='2 layers'):
        enc.steps(x, x, rows, TemporalCache(2, 2, 64, 'cpu'), 3)
    layer, att = enc.layers[0], enc.layers[0].self_attn
    slot, off, pos = (torch.zeros(k, dtype=torch.int32) for k in (5, 5, 2))
    for call in (lambda: layer.steps(x, x, slot, off, c.k[0], c.v[0], pos, 3, True),
                 lambda: att.steps(x, x, slot, off, c.k[0], c.v[0], pos, 3, ring=True)):
        with pytest.raises(L.OcoccError, match='CPU tensor'):
            call()
    with pytest.raises(RuntimeError, match='inference only'):
        enc.train().steps(x, x, rows, c, 3)


@pytest.fixture(scope='module')
def model():
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (register)
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    return DETECTORS.build(ococcnet_model_cfg()).eval()


def _tracklet(num):
    from objectcentricocccompletion_amd.tracklet import Tracklet
    return Tracklet(torch.ones(num, 7), list(range(num)), torch.ones(num), type=0)


def test_online_chunk_validation(model):
    """an int >= 1, default 1; anything else is a ValueError before the cache is built or a tensor looked at.  A valid value
    gets as far as the CPU-tensor check."""
    from objectcentricocccompletion_amd import _lib as L
    rh = model.roi_head
    pts = (torch.zeros(1, 3), torch.zeros(1, 7), torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long))
    assert 'online_chunk' not in rh.test_cfg and rh.online_chunk() == 1
    try:
        for bad in (0, -3, 2.0, '4', None, True, [2]):
            rh.test_cfg['online_chunk'] = bad
            with pytest.raises(ValueError, match='online_chunk'):
                rh.online_chunk()
            with pytest.raises(ValueError, match='online_chunk'):
                rh.simple_test_online(*pts, None, [_tracklet(4)])
        for good in (1, 3, 1000):
            rh.test_cfg['online_chunk'] = good
            assert rh.online_chunk() == good
            with pytest.raises(L.OcoccError, match='CPU tensor'):
                rh.simple_test_online(*pts, None, [_tracklet(4)])
    finally:
        del rh.test_cfg['online_chunk']


def test_steps_refusals_of_the_heads(model):
    """forward_steps keeps the three refusals of forward_step; simple_test_steps reports the slot list and CPU tensors on the
    host and leaves the state as it was"""
    from objectcentricocccompletion_amd import _lib as L
    rh, head = model.roi_head, model.roi_head.bbox_head
    state = rh.online_begin(3, 'cpu', cap=4)
    pts = (torch.zeros(1, 3), torch.zeros(1, 7), torch.zeros(1, dtype=torch.long))
    rows = (torch.ones(3, 7), torch.ones(3), torch.zeros(3, dtype=torch.long))
    with pytest.raises(L.OcoccError, match='not consecutive'):
        rh.simple_test_steps(*pts, *rows, [0, 1, 0], state)
    with pytest.raises(L.OcoccError, match='outside 0..2'):
        rh.simple_test_steps(*pts, *rows, [0, 0, 3], state)
    state.cache.pos_host[2] = 2
    with pytest.raises(L.OcoccError, match='cap = 4'):
        rh.simple_test_steps(*pts, *rows, [2, 2, 2], state)
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        rh.simple_test_steps(*pts, *rows, [1, 1, 2], state)
    assert state.frames == [0, 0, 2]
    with pytest.raises(RuntimeError, match='inference only'):
        rh.train().simple_test_steps(*pts, *rows, [1, 1, 2], state)
    rh.eval()
    args = (None,) * 5 + ([0, 0], state.cache)
    with pytest.raises(RuntimeError, match='inference only'):
        head.train().forward_steps(*args)
    head.eval()
    for key, exc in (('allow_attn_future', ValueError), ('online_tuning', NotImplementedError)):
        head.test_cfg[key] = True if key == 'allow_attn_future' else dict(num_iter=1, downsample_size=-1, balance_sample=True)
        try:
            with pytest.raises(exc):
                head.forward_steps(*args)
        finally:
            del head.test_cfg[key]


def test_tool_flag():
    """tools/test.py --online-chunk T: needs --online and T >= 1"""
    spec = importlib.util.spec_from_file_location('ococc_tools_test_chunk', os.path.join(ROOT, 'tools', 'test.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ['cfg.py', 'ck.pth', '--eval', 'iou']
    assert tool.parse_args(base).online_chunk is None and tool.parse_args(base + ['--online']).online_chunk is None
    args = tool.parse_args(base + ['--online', '--online-chunk', '16'])
    assert args.online and args.online_chunk == 16
    assert tool.parse_args(base + ['--online', '--online-chunk', '1']).online_chunk == 1
    for bad in (['--online-chunk', '4'], ['--online', '--online-chunk', '0'], ['--online', '--online-chunk', '-2'],
                ['--online', '--online-chunk', 'x']):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
