"""Several sensor frames per online call, host side (no device): the numpy restatement of the many-cloud scene-rows
kernels (tests/scene_steps_ref.py) on hand-made cases, the host's frame-major plan, the two exports' declaration, binding,
argument checks and INTEGRATION.md rows, what scene_steps_rows and simple_test_scene_steps report before any launch, and
the replay tool's --chunk."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_rows_ref as R        # noqa: E402
import scene_steps_ref as RS      # noqa: E402
from objectcentricocccompletion_amd import _lib as L         # noqa: E402
from objectcentricocccompletion_amd import scene_rows as S   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {'ococc_scene_rows_frames_count': 16, 'ococc_scene_rows_frames_fill': 26}


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


def test_reference_keeps_frames_apart_and_the_callers_order():
    """one box given for two frames with different clouds, a second box in frame 0 only, the caller's rows not frame-major:
    every row holds its own frame's points, in that frame's order; the cap picks per row; counts stay uncapped"""
    box = np.array([[0, 0, 0, 2, 4, 2, 0.0], [0.5, 0, 0, 2, 4, 2, -0.2]], np.float32)
    a = np.array([[0.2, 0.1, 1.0, 1], [30, 0, 1, 2], [0.3, -0.2, 0.5, 3]], np.float32)                       # frame 0
    b = np.array([[40, 0, 1, 4], [0.1, 0.1, 0.4, 5], [-0.2, 0.3, 1.5, 6], [0, 0, 9, 7], [0.4, 0.4, 1, 8]], np.float32)   # frame 1
    points, sizes = np.concatenate([a, b]), [3, 5]
    crop, frame_rows = box[[0, 0, 1]], [1, 0, 0]                         # rows: box 0 in frame 1, box 0 in frame 0, box 1 in frame 0
    feats = np.arange(6, dtype=np.float32).reshape(3, 2)
    xyz, fe, row, counts = RS.scene_steps(points, sizes, crop, frame_rows, attr_dims=1, row_feats=feats)
    assert counts.tolist() == [3, 2, 2] and row.tolist() == [0, 0, 0, 1, 1, 2, 2]
    assert fe[:, 0].tolist() == [5, 6, 8, 1, 3, 1, 3]
    assert np.array_equal(fe[:, 1:], feats[row]) and np.array_equal(xyz, points[[4, 5, 7, 0, 2, 0, 2], :3].astype(np.float64))
    # each row is what the one-cloud restatement makes of its frame alone
    for i, f in enumerate(frame_rows):
        one = R.scene_rows([a, b][f], crop[i:i + 1], attr_dims=1, row_feats=feats[i:i + 1])
        assert np.array_equal(xyz[row == i], one[0]) and np.array_equal(fe[row == i], one[1]) and counts[i] == one[3][0]
    capped = RS.scene_steps(points, sizes, crop, frame_rows, cap=2, attr_dims=1)
    assert capped[3].tolist() == [3, 2, 2] and capped[2].tolist() == [0, 0, 1, 1, 2, 2]
    assert capped[1][:, 0].tolist() == [[5, 6, 8][j] for j, _ in R.even_pick(3, 2)] + [1, 3, 1, 3]
    shift = np.eye(4)[:3].reshape(1, 12).repeat(3, 0)
    shift[0, 3] = 100.0                                                  # row 0 only: x' = x + 100
    moved = RS.scene_steps(points, sizes, crop, frame_rows, transforms=shift, rng=[-10, -10, -10, 10, 10, 10], attr_dims=1)
    assert moved[3].tolist() == [0, 2, 2] and moved[2].tolist() == [1, 1, 2, 2]
    empty = RS.scene_steps(points, sizes, crop[:0], [], attr_dims=1)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 1) and empty[3].shape == (0,)


def test_frame_major_plan():
    order, offsets = S.frame_major([2, 0, 2, 1, 0, 2], 4)
    assert order == [1, 4, 3, 0, 2, 5] and offsets == [0, 2, 3, 6, 6]     # stable within a frame; frame 3 without rows
    assert S.frame_major([], 0) == ([], [0]) and S.frame_major([], 2) == ([], [0, 0, 0])
    assert S.frame_major([0, 0, 0], 1) == ([0, 1, 2], [0, 3])


def test_exports_are_declared_bound_and_documented():
    import ctypes
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ococc_hip.h')).read(), flags=re.S)
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name, nargs in EXPORTS.items():
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, header)
        assert m, f'{name} is not declared in ococc_hip.h'
        assert len(m.group(1).split(',')) == len(L.SIGNATURES[name][1]) == nargs, name
        assert hasattr(ctypes.CDLL(L.LIB_PATH), name) and hasattr(L.lib, name)
        assert any(f'`{name}`' in line and line.startswith('|') for line in integration.splitlines()), f'{name}: no INTEGRATION.md row'
    lib = L.lib
    # invalid arguments are reported, not thrown, before anything is dereferenced or launched; empty inputs are no error
    count = lambda N, C, n, F, mp, mb, wsb=0, counts=None: lib.ococc_scene_rows_frames_count(
        None, N, C, None, None, n, None, F, mp, mb, None, None, counts, None, wsb, None)
    assert count(5, 2, 3, 1, 5, 3) == -1 and b'3 columns' in lib.ococc_last_error()
    for bad in ((-1, 3, 3, 1, 0, 3), (5, 3, -1, 1, 5, 0), (5, 3, 3, -1, 5, 3), (5, 3, 3, 1, -1, 3), (5, 3, 3, 1, 5, -1)):
        assert count(*bad) == -1 and b'negative size' in lib.ococc_last_error(), bad
    assert count(1 << 31, 3, 3, 1, 5, 3) == -1 and count(5, 3, 1 << 31, 1, 5, 3) == -1 and b'2^31 - 1' in lib.ococc_last_error()
    assert count(5, 3, 3, 1, 6, 3) == -1 and count(5, 3, 3, 1, 5, 4) == -1 and b'max_frame' in lib.ococc_last_error()
    assert count(5, 3, 3, 65536, 5, 3) == -1 and b'65535' in lib.ococc_last_error()
    assert count(5, 3, 3, 1, 5, 3) == -1 and b'null pointer' in lib.ococc_last_error()
    assert count(0, 3, 3, 2, 0, 3) == -1 and b'null counts' in lib.ococc_last_error()
    assert count(5, 3, 0, 2, 5, 0) == 0 and count(0, 3, 0, 0, 0, 0) == 0 and count(5, 3, 0, 0, 0, 0) == 0
    fill = lambda N, C, n, F, mp, mb, a, k, cap, m=0: lib.ococc_scene_rows_frames_fill(
        None, N, C, None, None, n, None, F, mp, mb, None, None, a, None, k, None, cap, None, None, m, None, None, None, None, 0, None)
    assert fill(0, 5, 0, 0, 0, 0, 3, 0, -1) == -1 and b'attr_dims' in lib.ococc_last_error()
    assert fill(0, 5, 0, 0, 0, 0, -1, 0, -1) == -1 and fill(0, 5, 0, 0, 0, 0, 2, -1, -1) == -1
    assert fill(0, 5, 0, 0, 0, 0, 2, 5, 1 << 31) == -1 and b'max_points' in lib.ococc_last_error()
    assert fill(0, 5, 0, 0, 0, 0, 2, 5, -1, -1) == -1 and b'num_out' in lib.ococc_last_error()
    assert fill(0, 5, 0, 0, 0, 0, 2, 5, 1024) == 0 and fill(7, 5, 0, 3, 7, 0, 2, 5, -1) == 0 and fill(7, 5, 3, 0, 0, 0, 2, 5, -1) == 0
    assert fill(7, 5, 3, 2, 7, 3, 2, 5, -1, 4) == -1 and b'null pointer' in lib.ococc_last_error()
    # the workspace is sized by the LARGEST frame: the one-cloud rule with its point count
    assert lib.ococc_scene_rows_workspace_bytes(4097, 7) == 2 * 4 * 7 * 4
    ws = ctypes.c_int64(0)                                  # any non-null address: refused before it is used
    small = lambda wsb: lib.ococc_scene_rows_frames_count(1, 9000, 3, 1, 1, 7, 1, 3, 4097, 7, None, None, 1, ctypes.addressof(ws), wsb, None)
    assert small(2 * 4 * 7 * 4 - 1) == -1 and b'workspace too small' in lib.ococc_last_error()


def _frames(n=2, F=2):
    return dict(points=torch.zeros(4, 5), cloud_sizes=[4] + [0] * (F - 1), boxes=torch.ones(n, 7), scores=torch.ones(n))


def test_scene_steps_rows_reports_on_the_host():
    """everything but the device itself is checked before the device is asked for: the refusals are reached with CPU
    tensors, and correct arguments on CPU tensors end at the CPU-tensor report of every operator"""
    ok = _frames()
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        S.scene_steps_rows(**ok, frame_rows=[0, 1])
    for sizes in ([3, 0], [5, 0], [5, -1], [4]):
        with pytest.raises(L.OcoccError, match='cloud_sizes' if len(sizes) == 2 else 'frame_rows'):
            S.scene_steps_rows(**dict(ok, cloud_sizes=sizes), frame_rows=[0, 1])
    for rows in ([0], [0, 1, 1], [0, 2], [-1, 0]):
        with pytest.raises(L.OcoccError, match='frame_rows'):
            S.scene_steps_rows(**ok, frame_rows=rows)
    with pytest.raises(L.OcoccError, match='65535'):
        S.scene_steps_rows(**dict(ok, cloud_sizes=[4] + [0] * 65535), frame_rows=[0, 1])
    # what scene_step_rows reports
    with pytest.raises(L.OcoccError, match='points must be'):
        S.scene_steps_rows(**dict(ok, points=torch.zeros(4, 4)), frame_rows=[0, 1])
    with pytest.raises(L.OcoccError, match='boxes must be'):
        S.scene_steps_rows(**dict(ok, boxes=torch.ones(2, 6)), frame_rows=[0, 1])
    with pytest.raises(L.OcoccError, match='scores'):
        S.scene_steps_rows(**dict(ok, scores=torch.ones(3)), frame_rows=[0, 1])
    with pytest.raises(L.OcoccError, match='transforms'):
        S.scene_steps_rows(**ok, frame_rows=[0, 1], transforms=torch.zeros(2, 9))
    with pytest.raises(L.OcoccError, match='point_cloud_range'):
        S.scene_steps_rows(**ok, frame_rows=[0, 1], point_cloud_range=[0, 0, 1])
    with pytest.raises(L.OcoccError, match='max_points'):
        S.scene_steps_rows(**ok, frame_rows=[0, 1], max_points=1 << 31)


def _step(n, F=3, **kw):
    base = dict(points=torch.zeros(6, 5), cloud_sizes=[2] * F, poses=np.stack([np.eye(4)] * F), boxes=torch.ones(n, 7),
                scores=torch.ones(n), labels=torch.zeros(n, dtype=torch.long))
    base.update(kw)
    return base


def test_scene_steps_reports_on_the_host(model):
    rh = model.roi_head
    state = rh.online_begin(4, 'cpu', cap=4)
    snapshot = lambda: (list(state.frames), [None if o is None else o.copy() for o in state.origin])
    before = snapshot()

    def same_state():
        now = snapshot()
        return now[0] == before[0] and all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(now[1], before[1]))

    for bad in (np.eye(4), np.zeros((2, 4, 4)), np.zeros((3, 3, 4)), np.full((3, 4, 4), np.nan), torch.full((3, 4, 4), float('inf'))):
        with pytest.raises(L.OcoccError, match='poses'):
            rh.simple_test_scene_steps(**_step(2, poses=bad), frame_rows=[0, 1], slot_rows=[0, 0], state=state)
    singular = np.stack([np.eye(4), np.zeros((4, 4)), np.eye(4)])
    with pytest.raises(L.OcoccError, match='singular'):
        rh.simple_test_scene_steps(**_step(2, poses=singular), frame_rows=[1, 2], slot_rows=[0, 0], state=state)
    # frame_rows: the wrong length, outside 0..F-1, and inside a slot's run going back or repeating a cloud
    for rows, what in (([0], 'frame_rows must'), ([0, 3, 1], 'frame_rows must'), ([-1, 0, 1], 'frame_rows must'),
                       ([1, 0, 2], 'strictly increasing'), ([0, 1, 1], 'strictly increasing'), ([2, 2, 0], 'strictly increasing')):
        with pytest.raises(L.OcoccError, match=what):
            rh.simple_test_scene_steps(**_step(3), frame_rows=rows, slot_rows=[1, 1, 1], state=state)
    # (a gap is fine, and so is a later slot that starts at an earlier cloud: the run ends at the CPU-tensor report)
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        rh.simple_test_scene_steps(**_step(3), frame_rows=[0, 2, 1], slot_rows=[1, 1, 3], state=state)
    assert same_state()
    # what check_steps refuses
    with pytest.raises(L.OcoccError, match='not consecutive'):
        rh.simple_test_scene_steps(**_step(3), frame_rows=[0, 0, 1], slot_rows=[1, 2, 1], state=state)
    with pytest.raises(L.OcoccError, match='outside 0..3'):
        rh.simple_test_scene_steps(**_step(1), frame_rows=[0], slot_rows=[4], state=state)
    with pytest.raises(L.OcoccError, match='do not fit'):
        rh.simple_test_scene_steps(**_step(5, F=5, points=torch.zeros(10, 5)), frame_rows=[0, 1, 2, 3, 4], slot_rows=[0] * 5, state=state)
    # a slot in mid-tracklet without an origin was stepped through simple_test_step(s): its fixed frame is not known here
    state.cache.pos_host[2] = 1
    before = snapshot()
    with pytest.raises(L.OcoccError, match='no origin'):
        rh.simple_test_scene_steps(**_step(3), frame_rows=[0, 1, 1], slot_rows=[0, 0, 2], state=state)
    assert same_state()                                              # slot 0 started in the refused call: nothing kept
    state.origin[2] = np.eye(4)
    before = snapshot()
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        rh.simple_test_scene_steps(**_step(3), frame_rows=[0, 1, 1], slot_rows=[0, 0, 2], state=state)
    with pytest.raises(L.OcoccError, match='scores'):
        rh.simple_test_scene_steps(**_step(3, scores=torch.ones(2)), frame_rows=[0, 1, 1], slot_rows=[0, 0, 2], state=state)
    assert same_state()
    import inspect
    assert 'merged' not in inspect.signature(rh.simple_test_scene_steps).parameters
    assert inspect.signature(rh.simple_test_steps).parameters['occ_transforms'].default is None
    model.train()
    try:
        with pytest.raises(RuntimeError, match='inference only'):
            rh.simple_test_scene_steps(**_step(1), frame_rows=[0], slot_rows=[0], state=state)
    finally:
        model.eval()


def test_replay_tool_chunk_arguments():
    import importlib.util
    spec = importlib.util.spec_from_file_location('ococc_tools_online_raw', os.path.join(ROOT, 'tools', 'online_raw.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ['cfg.py', 'ck.pth', 'raw.yaml']
    assert tool.parse_args(base).chunk == 1 and tool.parse_args(base + ['--chunk', '16']).chunk == 16
    assert tool.parse_args(base + ['--chunk', '3', '--save-occ', 'd']).save_occ == 'd'
    assert tool.parse_args(base + ['--chunk', '1', '--save-merged', 'd']).save_merged == 'd'
    for bad in (['--chunk', '0'], ['--chunk', '-2'], ['--chunk', '2', '--save-merged', 'd']):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
    import inspect
    assert inspect.signature(tool.replay).parameters['chunk'].default == 1
    for bad in (dict(chunk=0), dict(chunk=2, save_merged='d')):
        with pytest.raises(ValueError, match='chunk'):
            tool.replay(None, 'nothing.yaml', **bad)
