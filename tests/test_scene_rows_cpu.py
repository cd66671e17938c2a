"""Online inference from whole-scene clouds, host side (no device): the numpy restatement of csrc/scene_rows.hip
(tests/scene_rows_ref.py) on crafted inputs, the even pick of the cap over a grid of (members, cap), the two exports'
declaration, binding and INTEGRATION.md row, and what scene_step_rows and simple_test_scene_step report before any launch."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_rows_ref as R        # noqa: E402
from objectcentricocccompletion_amd import scene_rows as S   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {'ococc_scene_rows_workspace_bytes': 2, 'ococc_scene_rows_count': 11, 'ococc_scene_rows_fill': 19}


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


def test_even_pick_keeps_cap_rows_in_order():
    """every (m, cap) with m in 0..40, cap in 1..12: min(m, cap) rows, ascending members, the places 0..min(m, cap)-1 once
    each and in order; the package's own even_pick is the same function"""
    for m in range(41):
        for cap in range(1, 13):
            pick = R.even_pick(m, cap)
            assert pick == S.even_pick(m, cap)
            members, places = [j for j, _ in pick], [p for _, p in pick]
            assert len(pick) == min(m, cap), (m, cap)
            assert members == sorted(set(members)) and all(0 <= j < m for j in members)
            assert places == list(range(min(m, cap))), (m, cap, places)
    assert R.even_pick(7, -1) == R.even_pick(7, 0) == [(j, j) for j in range(7)]
    assert [j for j, _ in R.even_pick(10, 5)] == [1, 3, 5, 7, 9] and [j for j, _ in R.even_pick(3, 1)] == [2]


def test_reference_membership_faces_and_specials():
    """a box with yaw = -pi/2 (rot = yaw + pi/2 rounds to -4.4e-8: with dy == 0 the local x is dx exactly): the faces at
    local x = +-l/2 are outside, one ulp inside is inside; z = centre +- h/2 is inside, the next f32 distance beyond (3 + ulp,
    1 - 2^-22: |z - 2| = 1 + 2^-22 exactly) outside; a NaN x or y and infinite coordinates are in no box, a NaN z passes the height test, which is written
    ``!(|dz| > h/2)`` there -- the range filter is what drops such a point"""
    box = np.array([10, 5, 1, 2, 4, 2, -np.pi / 2], np.float32)            # centre z = 2, l/2 = 2, h/2 = 1
    f = np.float32
    pts = np.array([[12, 5, 2], [8, 5, 2], [np.nextafter(f(12), f(0)), 5, 2], [np.nextafter(f(8), f(20)), 5, 2],
                    [10, 5, 3], [10, 5, 1], [10, 5, np.nextafter(f(3), f(9))], [10, 5, f(1) - f(2.0 ** -22)],
                    [np.nan, 5, 2], [10, np.nan, 2], [10, 5, np.nan], [np.inf, 5, 2], [10, -np.inf, 2], [10, 5, np.inf]], f)
    assert R.in_box(pts, box).tolist() == [False, False, True, True, True, True, False, False] + [False, False, True, False, False, False]
    # a point in two overlapping boxes is a row of both; a box without points has count 0
    boxes = np.array([[0, 0, 0, 2, 4, 2, 0.3], [0.5, 0, 0, 2, 4, 2, -0.2], [50, 50, 0, 2, 4, 2, 0]], np.float32)
    cloud = np.array([[0.2, 0.1, 1.0, 7, 8], [30, 0, 1, 9, 10], [0.3, -0.2, 0.5, 11, 12]], np.float32)
    feats = np.arange(6, dtype=np.float32).reshape(3, 2)
    xyz, fe, row, counts = R.scene_rows(cloud, boxes, attr_dims=2, row_feats=feats)
    assert counts.tolist() == [2, 2, 0] and row.tolist() == [0, 0, 1, 1]
    assert np.array_equal(xyz, cloud[[0, 2, 0, 2], :3].astype(np.float64))
    assert np.array_equal(fe, np.array([[7, 8, 0, 1], [11, 12, 0, 1], [7, 8, 2, 3], [11, 12, 2, 3]], np.float32))


def test_reference_transform_range_and_cap():
    rng = np.random.default_rng(3)
    box = np.array([[0, 0, -1, 4, 4, 4, 0.0]], np.float32)
    cloud = np.concatenate([rng.uniform(-1, 1, (20, 3)), rng.random((20, 2))], 1).astype(np.float32)
    ident = np.eye(4)[:3].reshape(1, 12)
    shift = ident.copy()
    shift[0, 3] = 100.0                                                     # x' = x + 100
    a = R.scene_rows(cloud, box, attr_dims=2)
    b = R.scene_rows(cloud, box, transforms=ident, attr_dims=2)
    c = R.scene_rows(cloud, box, transforms=shift, attr_dims=2)
    assert a[3].tolist() == [20] and np.array_equal(a[0], b[0]) and np.array_equal(c[0], a[0] + [100.0, 0, 0])
    assert (R.transform_bound(cloud[:, :3], shift[0])[:, 0] >= 3 * 2.0 ** -24 * 99).all()
    # the range is part of membership (counts) and is tested on the written xyz
    d = R.scene_rows(cloud, box, transforms=shift, rng=[-10, -10, -10, 10, 10, 10], attr_dims=2)
    assert d[3].tolist() == [0] and len(d[0]) == 0
    e = R.scene_rows(cloud, box, rng=[0, -10, -10, 10, 10, 10], attr_dims=2)
    assert e[3].tolist() == [int((cloud[:, 0] > 0).sum())] and (e[0][:, 0] > 0).all()
    # the cap leaves counts alone and picks evenly
    g = R.scene_rows(cloud, box, cap=6, attr_dims=2)
    assert g[3].tolist() == [20] and np.array_equal(g[0], a[0][[j for j, _ in R.even_pick(20, 6)]]) and len(g[0]) == 6


def test_exports_are_declared_bound_and_documented():
    import ctypes
    from objectcentricocccompletion_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ococc_hip.h')).read(), flags=re.S)
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name, nargs in EXPORTS.items():
        m = re.search(r'\b(?:int|int64_t)\s+%s\s*\(([^;]*)\)\s*;' % name, header)
        assert m, f'{name} is not declared in ococc_hip.h'
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and hasattr(_lib.lib, name)
        assert any(f'`{name}`' in line and line.startswith('|') for line in integration.splitlines()), f'{name}: no INTEGRATION.md row'
    makefile = open(os.path.join(ROOT, 'objectcentricocccompletion_amd', 'csrc', 'Makefile')).read()
    assert 'scene_rows.hip' in makefile
    lib = _lib.lib
    assert lib.ococc_scene_rows_workspace_bytes(4097, 3) == 2 * 4 * 3 * 4 and lib.ococc_scene_rows_workspace_bytes(0, 3) == 0
    assert lib.ococc_scene_rows_workspace_bytes(-1, 3) == -1
    # invalid arguments are reported, not thrown, before anything is dereferenced or launched; empty inputs are no error
    count = lambda n, c, b, ws=None, wsb=0, counts=None: lib.ococc_scene_rows_count(None, n, c, None, b, None, None, counts, ws, wsb, None)
    assert count(5, 2, 3) == -1 and b'3 columns' in lib.ococc_last_error()
    assert count(-1, 3, 3) == -1 and count(1 << 31, 3, 3) == -1
    assert count(5, 3, 3) == -1 and b'null pointer' in lib.ococc_last_error()
    assert count(0, 3, 3) == -1 and b'null counts' in lib.ococc_last_error()
    assert count(5, 3, 0) == 0 and count(0, 3, 0) == 0
    fill = lambda n, c, b, a, k, cap: lib.ococc_scene_rows_fill(None, n, c, None, b, None, None, a, None, k, cap, None, None,
                                                                 None, None, None, None, 0, None)
    assert fill(0, 5, 0, 3, 0, -1) == -1 and b'attr_dims' in lib.ococc_last_error()
    assert fill(0, 5, 0, -1, 0, -1) == -1 and fill(0, 5, 0, 2, -1, -1) == -1
    assert fill(0, 5, 0, 2, 5, 1 << 31) == -1 and b'max_points' in lib.ococc_last_error()
    assert fill(0, 5, 0, 2, 5, 1024) == 0 and fill(7, 5, 0, 2, 5, -1) == 0
    assert fill(7, 5, 3, 2, 5, -1) == -1 and b'null pointer' in lib.ococc_last_error()


def test_scene_step_rows_refuses_cpu_tensors():
    from objectcentricocccompletion_amd import _lib as L
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        S.scene_step_rows(torch.zeros(4, 5), torch.ones(1, 7), torch.ones(1))
    # PointDecoration's expressions: the yaw divided in double precision, the sizes in f32
    boxes = torch.tensor([[0, 0, 0, 1.9, 4.7, 1.6, 2.5], [0, 0, 0, 2.1, 5.3, 1.7, -3.0]])
    deco = S.decoration(boxes, torch.tensor([0.25, 0.75]))
    want = torch.tensor([[float(b[6]) / 3.1415] + (b[3:6] / 10).tolist() + [s] for b, s in zip(boxes, (0.25, 0.75))])
    assert torch.equal(deco, want) and deco.dtype == torch.float32


def _scene_frame(n=1):
    return dict(points=torch.zeros(4, 5), pose=np.eye(4), boxes=torch.ones(n, 7), scores=torch.ones(n),
                labels=torch.zeros(n, dtype=torch.long))


def test_scene_step_reports_on_the_host(model):
    from objectcentricocccompletion_amd import _lib as L
    rh = model.roi_head
    state = rh.online_begin(3, 'cpu', cap=4)
    assert state.origin == [None, None, None]
    for bad in (np.eye(3), np.zeros((4, 4, 1)), np.full((4, 4), np.nan), torch.full((4, 4), float('inf'))):
        with pytest.raises(L.OcoccError, match='pose'):
            rh.simple_test_scene_step(**dict(_scene_frame(), pose=bad), slot=[0], state=state)
    with pytest.raises(L.OcoccError, match='singular'):
        rh.simple_test_scene_step(**dict(_scene_frame(), pose=np.zeros((4, 4))), slot=[0], state=state)
    with pytest.raises(L.OcoccError, match='duplicate'):
        rh.simple_test_scene_step(**_scene_frame(2), slot=[1, 1], state=state)
    # a slot in mid-tracklet without an origin was stepped through simple_test_step: its fixed frame is not known here
    state.cache.pos_host[2] = 1
    with pytest.raises(L.OcoccError, match='no origin'):
        rh.simple_test_scene_step(**_scene_frame(2), slot=[0, 2], state=state)
    assert state.origin == [None, None, None]                       # nothing kept from a refused step
    # with an origin the step goes on to the device check (this state lives on the host) ...
    state.origin[2] = np.eye(4)
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        rh.simple_test_scene_step(**_scene_frame(2), slot=[0, 2], state=state)
    assert state.origin[0] is None and state.frames == [0, 0, 1]
    # ... and reset clears origins, per slot and all
    state.origin[0] = np.eye(4)
    state.reset([2])
    assert state.origin[2] is None and state.origin[0] is not None and state.frames == [0, 0, 0]
    state.reset()
    assert state.origin == [None, None, None]
    model.train()
    try:
        with pytest.raises(RuntimeError, match='inference only'):
            rh.simple_test_scene_step(**_scene_frame(1), slot=[0], state=state)
    finally:
        model.eval()


def test_scene_step_reports_lengths_before_the_device(model):
    """the order of host checks is the chunked call's: wrong lengths are reported before CPU tensors, and no refusal --
    lengths, device, a singular pose, a bad slot -- leaves anything in the state"""
    from objectcentricocccompletion_amd import _lib as L
    rh = model.roi_head
    state = rh.online_begin(3, 'cpu', cap=4)
    state.cache.pos_host[1], state.origin[1] = 2, np.eye(4)
    origin, frames = list(state.origin), list(state.frames)
    same = lambda: state.frames == frames and all(a is b for a, b in zip(state.origin, origin))
    for bad in (dict(scores=torch.ones(3)), dict(labels=torch.zeros(1, dtype=torch.long)), dict(boxes=torch.ones(3, 7))):
        with pytest.raises(L.OcoccError, match=r'2 slots, \d scores, \d labels for \d boxes'):
            rh.simple_test_scene_step(**dict(_scene_frame(2), **bad), slot=[0, 1], state=state)
        assert same()
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        rh.simple_test_scene_step(**_scene_frame(2), slot=[0, 1], state=state)
    assert same()
    with pytest.raises(L.OcoccError, match='singular'):
        rh.simple_test_scene_step(**dict(_scene_frame(2), pose=np.diag([1.0, 1.0, 0.0, 1.0])), slot=[1, 0], state=state)
    assert same()
    with pytest.raises(L.OcoccError, match='outside'):
        rh.simple_test_scene_step(**_scene_frame(2), slot=[0, 3], state=state)
    assert same()


def test_replay_tool_arguments_and_cache_choice(model):
    import importlib.util
    from objectcentricocccompletion_amd import _lib as L
    spec = importlib.util.spec_from_file_location('ococc_tools_online_raw', os.path.join(ROOT, 'tools', 'online_raw.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.parse_args(['cfg.py', 'ck.pth', 'raw.yaml'])
    assert args.slots == 64 and args.out is None and args.poses is None
    with pytest.raises(SystemExit):
        tool.parse_args(['cfg.py', 'ck.pth', 'raw.yaml', '--slots', '0'])
    rh = model.roi_head
    assert tool.choose_cache(rh, 0) == dict(cap=1) and tool.choose_cache(rh, 256) == dict(cap=256)
    assert tool.choose_cache(rh, 257) == dict(cap=257, long=True)
    with pytest.raises(L.OcoccError, match='4096'):
        tool.choose_cache(rh, 4097)
    rh.test_cfg['attn_window_size'] = 16
    try:
        assert tool.choose_cache(rh, 5000) == dict(cap=16, ring=True) and tool.choose_cache(rh, 200) == dict(cap=200)
    finally:
        del rh.test_cfg['attn_window_size']
