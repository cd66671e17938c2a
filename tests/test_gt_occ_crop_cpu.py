"""Ground-truth occupancy export without a GPU: the operator-by-operator crop (bbox.crop_gt_occ_aten) against a float64
restatement of the reference's branch (tracklet_roi_head_occ.py:661-689 with check_pt_in_box3d of
roiaware_pool3d/src/points_in_boxes_cuda.cu:24-49), the faces of the box, the config check, the C declarations, the
--save-gt-occ flag and the files."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gt_occ_ref import face_case, random_case, restate_f64        # noqa: E402


def test_aten_crop_against_the_float64_restatement():
    from objectcentricocccompletion_amd import bbox
    cells, gt, roi = random_case(24, 1500, seed=5)
    pts, inside, dist = restate_f64(cells, gt, roi)
    clear = dist > 1e-4
    excluded = 1.0 - clear.mean()
    print(f'pairs within 1e-4 m of a face: {excluded:.5f}; inside: {inside.mean():.3f}')
    assert excluded <= 0.02
    assert 0.2 < inside.mean() < 0.9                                        # the crop does cut
    got = bbox.crop_gt_occ_aten(cells, gt, roi)
    assert len(got) == 24 and all(t.dtype == torch.float32 and t.dim() == 2 and t.size(1) == 3 for t in got)
    p32, in32 = bbox._gt_occ_points_mask(cells, gt, roi)
    assert [int(t.size(0)) for t in got] == in32.sum(1).tolist()
    assert np.array_equal(in32.numpy()[clear], inside[clear])
    err = np.abs(p32.double().numpy() - pts).max()
    print(f'largest deviation of the points: {err:.3e}')
    assert err <= 2e-5
    for n in (0, 7, 23):                                                    # cell order is kept
        assert torch.equal(got[n], p32[n][in32[n]])
    # the packed form on CPU tensors is the same chain, with the value column
    values = torch.linspace(0.1, 0.9, 24)
    packed, counts = bbox.crop_gt_occ_packed(cells, gt, roi, values)
    assert counts == [int(t.size(0)) for t in got] and torch.equal(packed[:, :3], torch.cat(got))
    assert torch.equal(packed[:, 3], values.repeat_interleave(torch.tensor(counts)))
    packed, _ = bbox.crop_gt_occ_packed(cells, gt, roi)
    assert packed.dtype == torch.float32 and bool((packed[:, 3] == 1).all())
    for c, g_, r_ in ((cells[:0], gt, roi), (cells, gt[:0], roi[:0])):
        packed, counts = bbox.crop_gt_occ_packed(c, g_, r_)
        assert tuple(packed.shape) == (0, 4) and counts == [0] * g_.size(0)


def test_cells_on_the_faces():
    from objectcentricocccompletion_amd import bbox
    cells, gt, roi, trig, keep = face_case()
    got = bbox.crop_gt_occ_aten(cells, gt, roi, trig=trig)
    exp = (cells + torch.tensor([8.0, -4.0, 2.0]))[torch.tensor(keep)]
    assert len(got) == 1 and torch.equal(got[0], exp)


def test_config_check():
    from objectcentricocccompletion_amd import config, heads, point_pool, roi_head  # noqa: F401 (registers)
    from objectcentricocccompletion_amd.registry import DETECTORS
    roi_head.check_save_gt_occ_cfg(dict(save_gt_occ=True, gt_occ_save_root='x'))
    roi_head.check_save_gt_occ_cfg(dict(save_gt_occ=False, tta=dict(merge='max')))
    roi_head.check_save_gt_occ_cfg(dict(save_occ=True))                       # (not this check's key)
    roi_head.check_save_gt_occ_cfg(None)
    with pytest.raises(ValueError, match='gt_occ_save_root'):
        roi_head.check_save_gt_occ_cfg(dict(save_gt_occ=True))
    with pytest.raises(ValueError, match='gt_occ_save_root'):
        roi_head.check_save_gt_occ_cfg(dict(save_gt_occ=True, occ_save_root='x'))
    with pytest.raises(ValueError, match='tta'):
        roi_head.check_save_gt_occ_cfg(dict(save_gt_occ=True, gt_occ_save_root='x', tta=dict(merge='max')))
    cfg = config.fromfile(os.path.join(ROOT, 'configs', 'ococcnet_mi355x.py'))
    config.merge_from_dict(cfg, {'model.test_cfg.save_gt_occ': True})
    with pytest.raises(ValueError, match='gt_occ_save_root'):                 # refused when the head is built
        DETECTORS.build(cfg['model'])


def test_files_round_trip(tmp_path):
    """a hand-made packed array (frames of 2, 0 and 3 cells, score 1) through the writer and the frame reader"""
    from objectcentricocccompletion_amd import occ_export
    packed = np.array([[1.0, 2.0, 3.0, 1.0], [4.0, 5.0, 6.0, 1.0], [-7.5, 8.25, 0.5, 1.0], [9.0, -1.0, 2.0, 1.0],
                       [0.125, 0.25, 0.5, 1.0]], np.float32)
    counts, ts = [2, 0, 3], [1553629304780200, 1553629304880200, 1553629305080200]
    paths = occ_export.write_tracklet_occ(str(tmp_path), 'segment-1_with_camera_labels', ts, 1, 'obj_7', packed, counts)
    assert paths == [f'{tmp_path}/segment-1_with_camera_labels/{t}/1_obj_7.bin' for t in ts]
    assert [os.path.getsize(p) for p in paths] == [32, 0, 48]
    cuts = [0, 2, 2, 5]
    for i, t in enumerate(ts):
        a = occ_export.load_frame_occ(str(tmp_path), 'segment-1_with_camera_labels', t)
        assert a.dtype == np.float32 and a.tobytes() == packed[cuts[i]:cuts[i + 1]].tobytes()
        assert np.all(a[:, 3] == 1)
    assert occ_export.load_frame_occ(str(tmp_path), 'segment-1_with_camera_labels', ts[0] + 1).shape == (0, 4)


EXPORTS = ('ococc_gt_occ_crop_count', 'ococc_gt_occ_crop_fill')


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
    assert 'tracklet_roi_head_occ.py:634-702' in header and 'points_in_boxes_cuda.cu:24-49' in header


def test_exports_check_their_arguments_before_any_launch():
    from objectcentricocccompletion_amd import _lib as L
    lib = L.lib
    tiles = lib.ococc_gt_occ_crop_tiles
    assert [tiles(3, k) for k in (0, 1, 1024, 1025, 2049)] == [0, 3, 3, 6, 9] and tiles(0, 500) == 0 and tiles(-1, 5) == 0
    count = lambda K, N, ld=7, t=None: lib.ococc_gt_occ_crop_count(None, K, None, ld, None, 7, N, None, None, None, None,
                                                                   None, tiles(N, K) if t is None else t, None, None)
    fill = lambda K, N, ld=7, t=None, n_out=0: lib.ococc_gt_occ_crop_fill(None, K, None, 7, None, ld, N, None, None, None,
                                                                          None, None, tiles(N, K) if t is None else t,
                                                                          None, None, n_out, None)
    assert count(0, 0) == 0 and count(100, 0) == 0 and fill(0, 0) == 0 and fill(0, 5) == 0 and fill(100, 0) == 0
    assert count(-1, 2) == -1 and b'K < 0' in lib.ococc_last_error()
    assert count(10, 2, ld=6) == -1 and b'stride' in lib.ococc_last_error()
    assert fill(10, 2, ld=6) == -1 and b'stride' in lib.ococc_last_error()
    assert count(2000, 3, t=3) == -1 and b'tiles' in lib.ococc_last_error()
    assert fill(2000, 3, t=7, n_out=5) == -1 and b'tiles' in lib.ococc_last_error()
    assert count(10, 2) == -1 and b'null pointer' in lib.ococc_last_error()
    assert fill(10, 2, n_out=0) == 0                                          # nothing kept: nothing to launch
    assert fill(10, 2, n_out=4) == -1 and b'null pointer' in lib.ococc_last_error()
    with pytest.raises(L.OcoccError, match='n_out'):
        L.check(fill(10, 2, n_out=-1), 'gt_occ_crop_fill')


def test_kernel_binding_refuses_cpu_tensors():
    from objectcentricocccompletion_amd import bbox
    from objectcentricocccompletion_amd._lib import OcoccError
    cells, gt, roi, trig, _ = face_case()
    with pytest.raises(OcoccError, match='no CPU fallback'):
        bbox.gt_occ_crop_kernels(cells, gt, roi, *trig)


def test_test_tool_lists_the_flag():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), '--help'], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and '--save-gt-occ DIR' in out.stdout
    import importlib.util
    spec = importlib.util.spec_from_file_location('ococc_tools_test', os.path.join(ROOT, 'tools', 'test.py'))
    test_tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(test_tool)
    args = test_tool.parse_args(['cfg.py', 'ck.pth', '--save-gt-occ', 'some/dir'])
    assert args.save_gt_occ == 'some/dir' and args.save_occ is None
    assert test_tool.parse_args(['cfg.py', 'ck.pth', '--eval', 'iou']).save_gt_occ is None
