"""Online inference past 256 frames, host side (no device): the long / ring form of the attention step
(csrc/causal_attn_step.hip, ococc_temporal_attention_step_long_f32) is declared, bound and documented and reports argument
errors before it dereferences or launches anything; the bookkeeping of a ring and of a long TemporalCache; the window a ring
cache cannot serve and the tracklet no cache holds are reported on the host."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'ococc_temporal_attention_step_long_f32'


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
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == len(_lib.SIGNATURES[NAME][1]) == 21
    old = _lib.SIGNATURES['ococc_temporal_attention_step_f32'][1]
    assert _lib.SIGNATURES[NAME][1] == old[:17] + [ctypes.c_int32] + old[17:]      # ``ring`` after ``window``
    assert args[16] == 'int32_t window' and args[17] == 'int32_t ring'
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME) and hasattr(_lib.lib, NAME)
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert any(f'`{NAME}`' in line and line.startswith('|') for line in integration.splitlines()), 'no INTEGRATION.md row'


def test_header_bindings_and_integration_agree_on_the_exports():
    """every function the header declares is bound and named in INTEGRATION.md, and nothing is bound that is not declared"""
    from objectcentricocccompletion_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ococc_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(ococc_[a-z0-9_]+)\s*\(', header))
    assert NAME in declared and declared == set(_lib.SIGNATURES)
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert f'`{NAME}`' in integration and '`ococc_temporal_attention_step_f32`' in integration


def _call(cap=8, D=8, window=0, ring=0, n=1, slots=1, ptr=None):
    from objectcentricocccompletion_amd import _lib
    return _lib.lib.ococc_temporal_attention_step_long_f32(ptr, 8, ptr, 8, ptr, 8, ptr, ptr, ptr, ptr, n, slots, cap, 1, D, 1.0,
                                                           window, ring, ptr, 8, None)


def test_argument_errors_are_reported_before_anything_is_touched():
    """every call passes null pointers: a check that ran after a dereference or a launch would not return"""
    from objectcentricocccompletion_amd import _lib
    err = _lib.lib.ococc_last_error
    assert _call(cap=4097) == -1 and b'4096' in err()
    for window in (0, -1, 9):
        assert _call(cap=8, window=window, ring=1) == -1 and b'ring' in err(), window
    assert _call(cap=4097, window=0, ring=1) == -1 and b'4096' in err()
    assert _call(D=6) == -1 and b'multiple of 4' in err()
    assert _call(D=388) == -1
    assert _call(n=2, slots=1) == -1 and b'more rows' in err()
    for kw in (dict(), dict(cap=4096), dict(cap=8, window=8, ring=1), dict(cap=8, window=1, ring=1), dict(cap=300, window=3)):
        assert _call(**kw) == -1 and b'null pointer' in err(), kw          # valid sizes: the pointers are what is wrong
    with pytest.raises(_lib.OcoccError):
        _lib.check(_call(), 'temporal_attention_step_long')
    assert _call(n=0) == 0                                                   # an empty step is no error


def test_ring_and_long_cache_bookkeeping():
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ.layers import TemporalCache
    c = TemporalCache(3, 2, 64, 'cpu', cap=2, ring=True)
    assert c.ring and c.long and c.k[0].shape == (2, 2, 64) and c.nbytes() == 2 * 3 * 2 * 2 * 64 * 4
    c.pos_host[:] = [2, 1000]
    assert c.check_step([0, 1]) == [0, 1]                                    # a ring slot is never full
    slot = torch.tensor([1], dtype=torch.int32)
    c.advance([1], slot)
    assert c.pos_host == [2, 1001] and c.pos.tolist() == [0, 1]
    c.pos_host[1] = 2 ** 31 - 2
    assert c.check_step([1]) == [1]
    c.pos_host[1] = 2 ** 31 - 1
    with pytest.raises(L.OcoccError, match='2\\*\\*31'):
        c.check_step([1])
    with pytest.raises(L.OcoccError, match='duplicate'):
        c.check_step([0, 0])
    c.reset([1])
    assert c.pos_host == [2, 0] and c.check_step([1]) == [1]
    c.reset()
    assert c.pos_host == [0, 0] and c.pos.tolist() == [0, 0]
    assert TemporalCache(3, 1, 1536, 'cpu', cap=16, ring=True).nbytes() == 589824   # the ococcnet model, W = 16: 0.6 MB

    long = TemporalCache(1, 1, 8, 'cpu', cap=300, long=True)
    assert long.long and not long.ring and long.k[0].shape == (1, 300, 8)
    long.pos_host[0] = 299
    assert long.check_step([0]) == [0]
    long.pos_host[0] = 300
    with pytest.raises(L.OcoccError, match='cap = 300'):
        long.check_step([0])
    assert TemporalCache(1, 1, 4, 'cpu', cap=4096, long=True).cap == 4096
    for kw in (dict(long=True), dict(ring=True)):
        with pytest.raises(L.OcoccError, match='4096'):
            TemporalCache(1, 1, 4, 'cpu', cap=4097, **kw)
        with pytest.raises(L.OcoccError):
            TemporalCache(1, 1, 4, 'cpu', cap=0, **kw)
    plain = TemporalCache(1, 1, 4, 'cpu')
    assert plain.cap == 256 and not plain.ring and not plain.long
    with pytest.raises(L.OcoccError, match='256'):
        TemporalCache(1, 1, 4, 'cpu', cap=257)                               # the default form keeps its limit


def test_encoder_step_refuses_a_window_the_ring_cannot_serve():
    """reported before the CPU-tensor check, i.e. before anything could be launched; a window the ring serves gets as far
    as that check"""
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ.layers import SimpleEncoderLayer, TemporalCache, TransformerEncoder
    enc = TransformerEncoder(SimpleEncoderLayer(64, 4, dim_feedforward=32), 3).eval()
    c = TemporalCache(3, 2, 64, 'cpu', cap=3, ring=True)
    x = torch.zeros(2, 64)
    for window in (-1, 0, 4):
        with pytest.raises(L.OcoccError, match='ring'):
            enc.step(x, x, [0, 1], c, window)
    with pytest.raises(L.OcoccError, match='ring'):
        enc.step(x, x, [0, 1], c)                                            # (the default window is -1)
    c.pos_host[:] = [7, 1000]                                                # past cap: no "full slot" either
    for window in (1, 3):
        with pytest.raises(L.OcoccError, match='CPU tensor'):
            enc.step(x, x, [0, 1], c, window)
    assert c.pos_host == [7, 1000]
    long = TemporalCache(3, 2, 64, 'cpu', cap=300, long=True)
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        enc.step(x, x, [0, 1], long)                                         # a long cache takes any window
    layer, att = enc.layers[0], enc.layers[0].self_attn
    slot, pos = torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    for call in (lambda: layer.step(x, x, slot, c.k[0], c.v[0], pos, 3, True, True),
                 lambda: att.step(x, x, slot, c.k[0], c.v[0], pos, 3, ring=True)):
        with pytest.raises(L.OcoccError, match='CPU tensor'):
            call()


@pytest.fixture(scope='module')
def model():
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (register)
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    return DETECTORS.build(ococcnet_model_cfg()).eval()


def test_online_begin_passes_the_flags(model):
    rh = model.roi_head
    ring = rh.online_begin(2, 'cpu', cap=3, ring=True).cache
    assert ring.ring and ring.long and ring.cap == 3 and ring.slots == 2 and ring.num_layers == 3
    long = rh.online_begin(1, 'cpu', cap=300, long=True).cache
    assert long.long and not long.ring and long.cap == 300
    plain = rh.online_begin(1, 'cpu').cache
    assert plain.cap == 256 and not plain.ring and not plain.long


def _tracklet(num):
    from objectcentricocccompletion_amd.tracklet import Tracklet
    return Tracklet(torch.ones(num, 7), list(range(num)), torch.ones(num), type=0)


def test_simple_test_online_chooses_the_cache_by_length_and_window(model):
    """4097 frames without a window: refused, naming the limit.  Everything shorter, and any length with a window, gets past
    that check to the CPU-tensor one, and the cache it would step through is the ring / long one."""
    from objectcentricocccompletion_amd import _lib as L
    rh = model.roi_head
    pts = (torch.zeros(1, 3), torch.zeros(1, 7), torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long))
    assert rh.test_cfg.get('attn_window_size', -1) <= 0
    with pytest.raises(L.OcoccError, match='4097 frames.*4096'):
        rh.simple_test_online(*pts, None, [_tracklet(4097)])
    for num in (4096, 257, 256):
        with pytest.raises(L.OcoccError, match='CPU tensor'):
            rh.simple_test_online(*pts, None, [_tracklet(num)])
    rh.test_cfg['attn_window_size'] = 16
    try:
        with pytest.raises(L.OcoccError, match='CPU tensor'):
            rh.simple_test_online(*pts, None, [_tracklet(4097)])
    finally:
        del rh.test_cfg['attn_window_size']
