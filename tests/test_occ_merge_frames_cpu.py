"""The occupancy-enhanced clouds of several frames per call, host side (no device): the numpy restatement
tests/occ_merge_frames_ref.py against occ_merge_ref, the operator chain occ_merge_frames_aten against it on CPU tensors,
what occ_ops.occ_merge_frames and the two frames exports refuse before any launch, the exports' declaration, binding and
INTEGRATION.md rows, simple_test_scene_steps_merged's refusals and the replay tool's --merged-per-call."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_merge_frames_ref as ref       # noqa: E402
import occ_merge_ref as one              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {'ococc_occ_merge_frames_count': 19, 'ococc_occ_merge_frames_fill': 24}
CASES = ref.cases()


@pytest.fixture(scope='module')
def model():
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (register)
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    cpu = torch.get_rng_state()
    m = DETECTORS.build(ococcnet_model_cfg()).eval()
    torch.set_rng_state(cpu)         # (later tests initialise networks from the global generator without seeding it)
    return m


def test_one_frame_is_the_single_frame_restatement():
    for c in one.cases():
        want, want_kept = one.occ_merge_ref(c['points'], c['occ'], c['counts'], c['use_dim'], c['row_score'], c['flags'],
                                            c['drop_observed'], c['score_threshold'])
        got, offsets, kept = ref.occ_merge_frames_ref(c['points'], [len(c['points'])], c['occ'], c['counts'],
                                                      [0] * len(c['counts']), c['use_dim'], c['row_score'], c['flags'],
                                                      c['drop_observed'], c['score_threshold'])
        assert got.tobytes() == want.tobytes() and got.shape == want.shape, c['name']
        assert offsets == [0, len(want)] and kept == want_kept, c['name']


def test_restatement_on_a_hand_written_example():
    """two clouds of 2 and 1 points, three rows: row 0 and row 2 of frame 1, row 1 of frame 0"""
    pts = np.arange(18, dtype=np.float32).reshape(3, 6)
    occ = np.array([[1, 2, 3, 0.5], [4, 5, 6, 0.1], [7, 8, 9, 0.9], [1, 1, 1, 0.3]], np.float32)
    f = np.float32
    merged, offsets, kept = ref.occ_merge_frames_ref(pts, [2, 1], occ, [1, 2, 1], [1, 0, 1], use_dim=3, score_threshold=0.2)
    assert offsets == [0, 3, 6] and kept == [1, 1, 1]
    assert merged.tolist() == [[0, 1, 2, 0, 0], [6, 7, 8, 0, 0], [7, 8, 9, f(0.9), 1],
                               [12, 13, 14, 0, 0], [1, 2, 3, f(0.5), 1], [1, 1, 1, f(0.3), 1]]
    merged, offsets, kept = ref.occ_merge_frames_ref(pts, [0, 3, 0], occ, [4], [2], use_dim=3, score_threshold=0.4)
    assert offsets == [0, 0, 3, 5] and kept == [2] and merged[3:, 3].tolist() == [f(0.5), f(0.9)]
    merged, offsets, kept = ref.occ_merge_frames_ref(pts[:0], [], occ[:0], [], [])
    assert merged.shape == (0, 7) and offsets == [0] and kept == []


def test_cases_cover_what_they_claim():
    by = {c['name']: c for c in CASES}
    want = {n: ref.occ_merge_frames_ref(*ref.args_of(c)) for n, c in by.items()}
    per_frame = lambda n: [sum(k for k, f in zip(want[n][2], by[n]['frame_rows']) if f == g) for g in range(len(by[n]['cloud_sizes']))]
    assert max(len(c['points']) for c in CASES) <= 6000 and max(len(c['occ']) for c in CASES) <= 12000
    c = by['interleaved']
    order = sorted(range(7), key=c['frame_rows'].__getitem__)
    assert order != list(range(7)) and order == [0, 3, 1, 5, 6, 2, 4]
    assert per_frame('interleaved')[0] == 0 and min(per_frame('interleaved')[1:]) > 0
    assert sorted(set(by['no_row_first']['frame_rows'])) == [1, 2] and sorted(set(by['no_row_middle']['frame_rows'])) == [0, 2]
    assert sorted(set(by['no_row_last']['frame_rows'])) == [0, 1]
    assert all(v > 0 for v in per_frame('no_row_last')[:2])
    dead = per_frame('dead_middle_frame')
    assert dead[1] == 0 and dead[0] > 0 and dead[2] > 0
    assert sum(want['all_survive'][2]) == sum(one.STRADDLE) and sum(want['none_survive'][2]) == 0
    assert sum(want['flags_drop1'][2]) < sum(want['flags_drop0'][2])
    assert sum(want['N0_cells'][2]) > 0 and len(by['N0_cells']['points']) == 0
    assert want['F0'][0].shape == (0, 7) and want['F0'][1] == [0]
    assert want['R0_F3'][1] == [0, 5, 5, 75]
    # the seams: real rows move down by the survivors in front; one seam is a copy-block edge, the others are not
    width = 7
    assert (ref.COPY_BLOCK * width) % ref.COPY_BLOCK == 0 and by['seam_on_block_edge']['cloud_sizes'][0] == ref.COPY_BLOCK
    assert per_frame('seam_on_block_edge')[0] > 0
    starts = np.cumsum(ref.SEAMS)[:-1] * width
    assert all(s % ref.COPY_BLOCK for s in starts) and any(s % 64 for s in starts)
    assert (sum(ref.SEAMS) * width) % ref.COPY_BLOCK != 0
    assert all(v > 0 for v in per_frame('seams'))


def test_chain_equals_the_restatement_on_the_host():
    from objectcentricocccompletion_amd.occ import occ_ops
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    for c in CASES:
        want, want_offsets, want_kept = ref.occ_merge_frames_ref(*ref.args_of(c))
        got, offsets, kept = occ_ops.occ_merge_frames_aten(
            t(c['points']), c['cloud_sizes'], t(c['occ']), c['counts'], c['frame_rows'], c['use_dim'], t(c['row_score']),
            t(c['flags']), c['drop_observed'], c['score_threshold'])
        assert isinstance(offsets, list) and offsets == want_offsets and kept == want_kept, c['name']
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape, c['name']
        assert got.numpy().tobytes() == want.tobytes(), c['name']


def test_operator_refuses_before_any_launch():
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ import occ_ops
    pts, occ = torch.zeros(4, 6), torch.zeros(5, 4)
    for fn in (occ_ops.occ_merge_frames, occ_ops.occ_merge_frames_aten):
        for bad in ((0, 1), tuple(range(6)) * 3, (0, 1, 6), (0, -1, 2), 7, 2):
            with pytest.raises(L.OcoccError, match='use_dim'):
                fn(pts, [4], occ, [5], [0], use_dim=bad)
        for counts in ([4], [2, 2], [6, -1], []):
            with pytest.raises(L.OcoccError, match='do not sum'):
                fn(pts, [4], occ, counts, [0] * len(counts))
        with pytest.raises(L.OcoccError, match='flags'):
            fn(pts, [4], occ, [5], [0], flags=torch.zeros(4, dtype=torch.uint8), drop_observed=True)
        with pytest.raises(L.OcoccError, match='row_score'):
            fn(pts, [4], occ, [2, 3], [0, 0], row_score=torch.zeros(3))
        with pytest.raises(L.OcoccError, match=r'\[M, 4\]'):
            fn(pts, [4], torch.zeros(5, 3), [5], [0])
        with pytest.raises(L.OcoccError, match=r'\[N, C\]'):
            fn(pts.double(), [4], occ, [5], [0])
        for sizes in ([3], [2, 3], [5, -1], []):
            with pytest.raises(L.OcoccError, match='cloud_sizes'):
                fn(pts, sizes, occ, [5], [0])
        with pytest.raises(L.OcoccError, match='65535'):
            fn(pts, [4] + [0] * 65535, occ, [5], [0])
        for rows in ([], [0, 0], [1], [-1], [2]):
            with pytest.raises(L.OcoccError, match='frame_rows'):
                fn(pts, [4], occ, [5], rows)
        with pytest.raises(L.OcoccError, match='frame_rows'):
            fn(pts, [1, 3], occ, [2, 3], [0, 2])
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        occ_ops.occ_merge_frames(pts, [1, 3], occ, [2, 3], [1, 0])
    assert occ_ops.merged_offsets([2, 0, 5], [2, 0, 2], [3, 4, 1]) == [0, 6, 6, 15]


def test_exports_are_declared_bound_and_documented():
    from objectcentricocccompletion_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'ococc_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name, nargs in EXPORTS.items():
        m = re.search(r'\b(?:int|int64_t)\s+%s\s*\(([^;]*)\)\s*;' % name, header)
        assert m, f'{name} is not declared in ococc_hip.h'
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and hasattr(_lib.lib, name)
        assert any(f'`{name}`' in line and line.startswith('|') for line in integration.splitlines()), f'{name}: no INTEGRATION.md row'
    lib = _lib.lib
    # invalid arguments are reported, not thrown, before anything is dereferenced or launched; empty parts are no error
    count = lambda M, R, tiles, F=1, N=0: lib.ococc_occ_merge_frames_count(
        None, M, None, None, None, R, None, None, F, N, None, None, 0, 0.0, None, None, tiles, None, None)
    assert count(-1, 0, 0) == -1 and count(0, -1, 0) == -1 and count(0, 0, 0, N=-1) == -1
    assert count(0, 0, 0, F=-1) == -1 and count(0, 0, 0, F=65536) == -1 and b'65535' in lib.ococc_last_error()
    assert count(0, 0, 0, F=0, N=3) == -1 and count(9, 2, 2, F=0) == -1 and b'F == 0' in lib.ococc_last_error()
    assert count(2048, 3, 4) == -1 and b'null pointer' in lib.ococc_last_error()
    assert b'ococc_occ_merge_frames_count' in lib.ococc_last_error()
    assert count(0, 0, 0) == 0 and count(7, 0, 0) == 0 and count(0, 0, 0, F=0) == 0 and count(0, 0, 0, F=65535, N=5) == 0
    one_table = (ctypes.c_int64 * 4)()
    tables = lambda M, R, tiles: lib.ococc_occ_merge_frames_count(
        None, M, None, one_table, one_table, R, one_table, one_table, 1, 0, None, None, 0, 0.0, None, None, tiles, None, None)
    assert tables(2048, 3, 4) == -1 and b'max_tiles' in lib.ococc_last_error()
    assert tables(2048, 3, 5) == -1 and b'null pointer' in lib.ococc_last_error()
    dims = lambda *v: (ctypes.c_int32 * len(v))(*v)
    fill = lambda N, C, use, D, M=0, R=0, K=0, tiles=0, F=1: lib.ococc_occ_merge_frames_fill(
        None, N, C, use, D, None, M, None, None, None, None, R, None, None, F, None, None, 0, 0.0, None, tiles, None, K, None)
    assert fill(0, 6, dims(0, 1), 2) == -1 and b'3 to 16' in lib.ococc_last_error()
    assert fill(0, 6, None, 3) == -1 and b'use_dim' in lib.ococc_last_error()
    assert fill(0, 6, dims(0, 1, 6), 3) == -1 and b'outside [0, C)' in lib.ococc_last_error()
    assert fill(-1, 6, dims(0, 1, 2), 3) == -1 and fill(0, 6, dims(0, 1, 2), 3, M=-1) == -1
    assert fill(0, 6, dims(0, 1, 2), 3, F=65536) == -1 and fill(4, 6, dims(0, 1, 2), 3, F=0) == -1
    assert fill(0, 6, dims(0, 1, 2), 3, M=4, R=1, K=5, tiles=1) == -1 and b'null pointer' in lib.ococc_last_error()
    assert fill(0, 6, dims(0, 1, 2), 3) == 0 and fill(0, 6, dims(0, 1, 2), 3, F=0) == 0
    assert fill(0, 6, dims(0, 1, 2, 3, 3), 5, M=9, R=2, K=0, tiles=2) == 0
    assert fill(5, 6, dims(0, 1, 2), 3) == -1 and b'null pointer' in lib.ococc_last_error()
    assert b'ococc_occ_merge_frames_fill' in lib.ococc_last_error()
    # the single-frame pair still names itself
    assert lib.ococc_occ_merge_count(None, -1, None, 0, None, None, 0, 0.0, None, None, 0, None, None) == -1
    assert b'ococc_occ_merge_count' in lib.ococc_last_error() and b'frames' not in lib.ococc_last_error()


def _call(n=1, F=2):
    return dict(points=torch.zeros(4, 5), cloud_sizes=[1, 3][:F], poses=np.stack([np.eye(4)] * F), boxes=torch.ones(n, 7),
                scores=torch.ones(n), labels=torch.zeros(n, dtype=torch.long), frame_rows=[0] * n, slot_rows=[0] * n)


def test_steps_merged_exists_and_refuses(model):
    from objectcentricocccompletion_amd import _lib as L
    rh = model.roi_head
    params = inspect.signature(rh.simple_test_scene_steps_merged).parameters
    assert list(params)[:9] == list(inspect.signature(rh.simple_test_scene_steps).parameters)[:9]
    assert params['merged'].default is True and 'occ' not in params and 'tune' in params and 'gt_rois' in params
    assert 'merged' not in inspect.signature(rh.simple_test_scene_steps).parameters
    assert 'simple_test_scene_steps_merged' in rh.simple_test_scene_steps.__doc__
    state = rh.online_begin(2, 'cpu', cap=4)
    step = lambda **kw: rh.simple_test_scene_steps_merged(**_call(), state=state, **kw)
    for bad in (dict(use_dims=5), dict(use_dim=2), dict(use_dim=[0, 1, -2]), dict(score_threshold='0'),
                dict(drop_observed=1), 1, 'yes', False, None):
        with pytest.raises(ValueError, match='merged'):
            step(merged=bad)
    with pytest.raises(L.OcoccError, match='use_dim'):
        step(merged=dict(use_dim=6))                   # the cloud has 5 columns
    rh.test_cfg['online_merged'] = dict(threshold=0.1)
    try:
        with pytest.raises(ValueError, match='online_merged'):
            step()
    finally:
        del rh.test_cfg['online_merged']
    # a right ``merged`` goes on to the checks of simple_test_scene_steps and the device check; nothing was kept
    with pytest.raises(L.OcoccError, match='cloud_sizes'):
        rh.simple_test_scene_steps_merged(**dict(_call(), cloud_sizes=[1, 2]), state=state)
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        step(merged=dict(use_dim=[0, 1, 2, 4], drop_observed=True))
    assert state.frames == [0, 0] and state.origin == [None, None]
    model.train()
    try:
        with pytest.raises(RuntimeError, match='inference only'):
            step()
    finally:
        model.eval()


def test_replay_tool_merged_per_call_arguments():
    import importlib.util
    spec = importlib.util.spec_from_file_location('ococc_tools_online_raw_frames', os.path.join(ROOT, 'tools', 'online_raw.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ['cfg.py', 'ck.pth', 'raw.yaml']
    assert tool.parse_args(base).merged_per_call is False
    args = tool.parse_args(base + ['--chunk', '4', '--save-merged', 'd', '--merged-per-call', '--merged-use-dim', '4'])
    assert args.merged_per_call is True and args.chunk == 4 and args.save_merged == 'd'
    assert tool.merged_arg(args) == dict(use_dim=4)
    assert tool.parse_args(base + ['--save-merged', 'd', '--merged-per-call']).chunk == 1
    for bad in (['--merged-per-call'], ['--chunk', '2', '--merged-per-call'], ['--chunk', '2', '--save-occ', 'd', '--merged-per-call'],
                ['--chunk', '2', '--save-merged', 'd']):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
    assert inspect.signature(tool.replay).parameters['merged_per_call'].default is False
    with pytest.raises(ValueError, match='chunk.*merged_per_call'):
        tool.replay(None, {}, chunk=2, save_merged='d')
    with pytest.raises(ValueError, match='merged_per_call'):
        tool.replay(None, {}, chunk=2, merged_per_call=True)
