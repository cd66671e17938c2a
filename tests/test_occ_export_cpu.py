"""Completed-occupancy files without a GPU: the writer / reader of occ_export.py, the C declarations, the operators'
refusal of CPU tensors and the --save-occ flag of tools/test.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _packed(counts, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((sum(counts), 4)).astype(np.float32)


def test_writer_reader_round_trip(tmp_path):
    from objectcentricocccompletion_amd import occ_export
    counts, ts = [3, 0, 5, 1], [100, 200, 300, 400]
    packed = _packed(counts)
    paths = occ_export.write_tracklet_occ(str(tmp_path), 'seg', ts, 1, 'abc', packed, counts)
    assert paths == [os.path.join(f'{tmp_path}/seg/{t}', '1_abc.bin') for t in ts]
    cuts = np.cumsum([0] + counts)
    for i, p in enumerate(paths):
        assert os.path.getsize(p) == counts[i] * 16
        a = occ_export.read_occ_bin(p)
        assert a.dtype == np.float32 and a.shape == (counts[i], 4)
        assert a.tobytes() == packed[cuts[i]:cuts[i + 1]].tobytes()
    # skipped frames are not written, the rows of the others stay theirs
    paths = occ_export.write_tracklet_occ(str(tmp_path / 'skip'), 'seg', ts, 1, 'abc', packed, counts, skip={0, 1})
    assert [os.path.relpath(p, tmp_path / 'skip') for p in paths] == ['seg/300/1_abc.bin', 'seg/400/1_abc.bin']
    assert np.array_equal(occ_export.read_occ_bin(paths[0]), packed[3:8])
    assert not os.path.exists(tmp_path / 'skip' / 'seg' / '100')
    with pytest.raises(AssertionError):
        occ_export.write_tracklet_occ(str(tmp_path), 'seg', ts, 1, 'abc', packed, [3, 0, 5])
    with pytest.raises(AssertionError):
        occ_export.write_tracklet_occ(str(tmp_path), 'seg', ts, 1, 'abc', packed[:-1], counts)
    with pytest.raises(AssertionError):
        occ_export.write_tracklet_occ(str(tmp_path), 'seg', ts, 1, 'abc', packed[:, :3], counts)


def test_layout_for_the_names_the_dataset_produces(tmp_path):
    """the reference's f"{root}/{segment_name}/{ts}/{type}_{id}.bin" with Waymo's segment names, integer microsecond
    timestamps, integer types and string ids (ids may hold underscores and dashes)"""
    from objectcentricocccompletion_amd import occ_export
    from objectcentricocccompletion_amd.tracklet import Tracklet
    seg = 'segment-10203656353524179475_7625_000_7645_000_with_camera_labels'
    trk = Tracklet(torch.zeros(2, 7), [1522688014970187, 1522688015069975], type=2, segment_name=seg, id='Wq_k-3x_ABC')
    paths = occ_export.write_tracklet_occ(str(tmp_path), trk.segment_name, trk.ts_list, trk.type, trk.id,
                                          _packed([2, 2]), [2, 2])
    assert paths[0] == f'{tmp_path}/{seg}/1522688014970187/2_Wq_k-3x_ABC.bin'
    assert paths[0] == occ_export.occ_path(str(tmp_path), seg, 1522688014970187, 2, 'Wq_k-3x_ABC')
    assert all(os.path.isfile(p) for p in paths)
    assert occ_export.load_frame_occ(str(tmp_path), seg, 1522688014970187, types=[2]).shape == (2, 4)
    assert occ_export.load_frame_occ(str(tmp_path), seg, 1522688014970187, types=[1]).shape == (0, 4)


def test_load_frame_occ_order_and_types(tmp_path):
    from objectcentricocccompletion_amd import occ_export
    root = str(tmp_path)
    objs = [(2, 'b', 3), (1, 'zz', 2), (1, 'a_1', 4), (4, 'c', 0)]
    data = {}
    for k, (type_, id_, n) in enumerate(objs):
        data[f'{type_}_{id_}.bin'] = _packed([n], seed=k)
        occ_export.write_tracklet_occ(root, 'seg', [7, 8], type_, id_, np.concatenate([data[f'{type_}_{id_}.bin']] * 2),
                                      [n, n], skip={1} if id_ == 'b' else None)
    with open(os.path.join(root, 'seg', '7', 'notes.txt'), 'w') as f:
        f.write('not an occupancy file')
    order = sorted(data)
    assert order == ['1_a_1.bin', '1_zz.bin', '2_b.bin', '4_c.bin']
    got = occ_export.load_frame_occ(root, 'seg', 7)
    assert got.dtype == np.float32 and np.array_equal(got, np.concatenate([data[n] for n in order]))
    assert np.array_equal(occ_export.load_frame_occ(root, 'seg', 7, types=[1]),
                          np.concatenate([data['1_a_1.bin'], data['1_zz.bin']]))
    assert np.array_equal(occ_export.load_frame_occ(root, 'seg', 7, types=('2', 4)), data['2_b.bin'])
    assert occ_export.load_frame_occ(root, 'seg', 8).shape == (6, 4)                 # 2_b was skipped in frame 8
    for missing in (occ_export.load_frame_occ(root, 'seg', 9), occ_export.load_frame_occ(root, 'other', 7),
                    occ_export.load_frame_occ(root, 'seg', 7, types=[3])):
        assert missing.dtype == np.float32 and missing.shape == (0, 4)


EXPORTS = ('ococc_dense_grid_cells_f32', 'ococc_occ_select_count', 'ococc_occ_select_fill')


def test_exports_declared_bound_and_documented():
    with open(os.path.join(ROOT, 'include', 'ococc_hip.h')) as f:
        header = f.read()
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
        integration = f.read()
    from objectcentricocccompletion_amd import _lib
    for name in EXPORTS:
        m = re.search(r'\bint %s\(([^;]*)\);' % name, header)
        assert m, f'{name} is not declared in include/ococc_hip.h'
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert callable(getattr(_lib.lib, name))
        assert f'`{name}`' in integration, f'{name} has no row in INTEGRATION.md'
    assert 'tracklet_roi_head_occ.py:612-745' in header and 'occ_ops.py:5-50' in header   # the reference lines replaced


def test_exports_check_their_arguments_before_any_launch():
    """the library's return codes: R == 0 is an empty result, a reversed cell range and a bad column count are
    OCOCC_EINVAL with a message (all decided on the host, in front of the first HIP call)"""
    from objectcentricocccompletion_amd import _lib as L
    lib = L.lib
    assert lib.ococc_dense_grid_cells_f32(None, None, None, 0, 0.2, 0, 0, None, None, None) == 0
    assert lib.ococc_dense_grid_cells_f32(None, None, None, 0, 0.2, 5, 4, None, None, None) == -1
    assert b'hi < lo' in lib.ococc_last_error()
    assert lib.ococc_dense_grid_cells_f32(None, None, None, 3, 0.2, 0, 10, None, None, None) == -1      # null pointers
    assert lib.ococc_occ_select_max_tiles(5000, 3) == 5000 // 1024 + 3
    assert lib.ococc_occ_select_count(None, 0, None, 0, 0.5, None, None, 0, None, None) == 0
    assert lib.ococc_occ_select_count(None, 5000, None, 3, 0.5, None, None, 6, None, None) == -1          # too few tiles
    assert b'max_tiles' in lib.ococc_last_error()
    fill = lambda R, cols, to_lidar=0: lib.ococc_occ_select_fill(None, 0, None, None, R, 0.5, None, R, None, None, 0.2,
                                                                 to_lidar, None, 0, None, None, None, cols, None, 0, None)
    assert fill(0, 3) == 0 and fill(0, 4) == 0
    assert fill(0, 5) == -1 and b'cols' in lib.ococc_last_error()
    assert fill(2, 3, to_lidar=1) == -1 and b'to_lidar' in lib.ococc_last_error()
    with pytest.raises(L.OcoccError, match='cols'):
        L.check(fill(0, 2), 'occ_select_fill')


def test_operators_refuse_cpu_tensors():
    from objectcentricocccompletion_amd._lib import OcoccError
    from objectcentricocccompletion_amd.occ import occ_ops
    sizes = torch.tensor([[1.0, 1.0, 1.0]])
    dims = torch.tensor([[5, 5, 5]], dtype=torch.int32)
    start = torch.tensor([0, 125])
    with pytest.raises(OcoccError, match='no CPU fallback'):
        occ_ops.dense_grid_cells(sizes, dims, start, 0.2, 0, 125, 125)
    with pytest.raises(OcoccError, match='no CPU fallback'):
        occ_ops.occ_select(torch.zeros(125), sizes, dims, start, 125, 0.2, 0.5)


def test_test_tool_lists_the_flag():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), '--help'], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and '--save-occ DIR' in out.stdout
    import importlib.util
    spec = importlib.util.spec_from_file_location('ococc_tools_test', os.path.join(ROOT, 'tools', 'test.py'))
    test_tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(test_tool)
    args = test_tool.parse_args(['cfg.py', 'ck.pth', '--save-occ', '/tmp/x'])
    assert args.save_occ == '/tmp/x' and test_tool.parse_args(['cfg.py', 'ck.pth', '--eval', 'iou']).save_occ is None


def test_save_occ_with_tta_is_refused_before_any_forward():
    """the augmented frames are not the frames to export: refused when the head is built, and by the check itself"""
    from objectcentricocccompletion_amd import config, heads, point_pool, roi_head  # noqa: F401 (registers)
    from objectcentricocccompletion_amd.registry import DETECTORS
    roi_head.check_save_occ_cfg(dict(save_occ=True, occ_save_root='x'))
    roi_head.check_save_occ_cfg(dict(save_occ=False, tta=dict(merge='max')))
    roi_head.check_save_occ_cfg(None)
    with pytest.raises(ValueError, match='tta'):
        roi_head.check_save_occ_cfg(dict(save_occ=True, occ_save_root='x', tta=dict(merge='max')))
    with pytest.raises(ValueError, match='occ_save_root'):
        roi_head.check_save_occ_cfg(dict(save_occ=True))
    cfg = config.fromfile(os.path.join(ROOT, 'configs', 'ococcnet_mi355x.py'))
    config.merge_from_dict(cfg, {'model.test_cfg.save_occ': True, 'model.test_cfg.occ_save_root': 'x',
                                 'model.test_cfg.tta': dict(merge='max')})
    with pytest.raises(ValueError, match='tta'):
        DETECTORS.build(cfg['model'])
