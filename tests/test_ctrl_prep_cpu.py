"""Tracklet data preparation (objectcentricocccompletion_amd/ctrl_prep.py, tools/ctrl/*), the part that needs no GPU:
configuration, host-side bookkeeping, and the three file formats pinned through WaymoTrackletDatasetWithOcc with the
device work replaced by restatements (numpy float64 membership; the C oracle's one-to-one IoU)."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from objectcentricocccompletion_amd import _lib as L  # noqa: E402
from objectcentricocccompletion_amd import ctrl_prep as cp  # noqa: E402
from objectcentricocccompletion_amd.tracklet import Tracklet  # noqa: E402

# our own text in the shape of the reference's tools/ctrl/data_configs/*.yaml (same keys, comments, list syntax)
REFERENCE_SHAPED_YAML = """\
# detection result in waymo bin format
bin_path: /somewhere/training/pred.bin
val_bin_path: /somewhere/validation/pred.bin
data_root: ./data/waymo/tracklet_data
exist_ok: False
# change the split for your need
split: training
#split: val
type: [1,] # 1:vehicle 2:pedestrian 4: cyclist

box:
  extra_width: 1

selection:
  mode: random
  size: 0.5

candidate:
  affinity_thresh: 0.5
"""


def in_box_f64(xyz, box):
    """check_pt_in_box3d in float64"""
    xyz, box = np.asarray(xyz, np.float64), np.asarray(box, np.float64)
    x, y, zb, w, l, h, yaw = box[:7]
    rot = yaw + np.pi / 2
    dx, dy = xyz[:, 0] - x, xyz[:, 1] - y
    lx = dx * np.cos(rot) - dy * np.sin(rot)
    ly = dx * np.sin(rot) + dy * np.cos(rot)
    return (np.abs(xyz[:, 2] - (zb + h / 2)) <= h / 2) & (lx > -l / 2) & (lx < l / 2) & (ly > -w / 2) & (ly < w / 2)


def crop_packed_f64(points, point_offsets, boxes, box_offsets):
    pts, bx = points.numpy(), boxes.numpy()
    idx = []
    for f in range(len(point_offsets) - 1):
        cloud = pts[point_offsets[f]:point_offsets[f + 1], :3]
        for b in range(box_offsets[f], box_offsets[f + 1]):
            idx.append(np.nonzero(in_box_f64(cloud, bx[b]))[0])
    counts = torch.tensor([len(i) for i in idx], dtype=torch.int64)
    return counts, torch.from_numpy(np.concatenate(idx) if idx else np.zeros(0, np.int64))


def max_iou_packed_oracle(pb, po, pf, gb, go, gf):
    from oracle import oracle as O
    pb, gb, pf, gf = pb.numpy(), gb.numpy(), pf.numpy(), gf.numpy()
    out = np.zeros((len(po) - 1, len(go) - 1), np.float32)
    for p in range(out.shape[0]):
        for g in range(out.shape[1]):
            fp, fg = pf[po[p]:po[p + 1]], gf[go[g]:go[g + 1]]
            common, ip, ig = np.intersect1d(fp, fg, return_indices=True)
            if len(common):
                out[p, g] = O.aligned_iou3d(pb[po[p]:po[p + 1]][ip], gb[go[g]:go[g + 1]][ig]).max()
    return torch.from_numpy(out)


def test_reference_shaped_yaml_parses(tmp_path):
    path = tmp_path / 'fsd_base_vehicle.yaml'
    path.write_text(REFERENCE_SHAPED_YAML)
    cfg, name = cp.load_config(str(path))
    assert name == 'fsd_base_vehicle' and cfg['split'] == 'training' and cfg['type'] == [1] and cfg['exist_ok'] is False
    assert cfg['box']['extra_width'] == 1 and cfg['candidate']['affinity_thresh'] == 0.5
    out = cp.output_paths(cfg, name)
    assert out['info'] == './data/waymo/tracklet_data/fsd_base_vehicle_training.pkl'
    assert out['database'] == './data/waymo/tracklet_data/fsd_base_vehicle_training_database'
    assert out['candidates'] == './data/waymo/tracklet_data/fsd_base_vehicle_training_gt_candidates.pkl'
    with pytest.raises(ValueError):
        cp.load_config(dict(cfg, name='x', split='train'))
    shipped, _ = cp.load_config(os.path.join(ROOT, 'tools', 'ctrl', 'data_configs', 'synthetic_vehicle.yaml'))
    assert set(cfg) <= set(shipped)


def test_split_selects_bin_and_velodyne_directory():
    cfg = dict(bin_path='a.bin', val_bin_path='b.bin', test_bin_path='c.bin')
    assert cp.bin_path_for_split(dict(cfg, split='training')) == 'a.bin'
    assert cp.bin_path_for_split(dict(cfg, split='val')) == 'b.bin'
    assert cp.bin_path_for_split(dict(cfg, split='test')) == 'c.bin'
    assert cp.velodyne_dir(dict(split='training')) == './data/waymo/kitti_format/training/velodyne'
    assert cp.velodyne_dir(dict(split='val')) == './data/waymo/kitti_format/training/velodyne'
    assert cp.velodyne_dir(dict(split='test', mm_data_root='/d')) == '/d/testing/velodyne'


def test_stride_selection():
    items = list(range(10))
    assert cp.select_tracklets(dict(selection=dict(mode='random', size=1.0)), items) == items
    assert cp.select_tracklets(dict(selection=dict(mode='random', size=0.5)), items) == items[::2]
    assert cp.select_tracklets(dict(selection=dict(mode='random', size=0.3)), items) == items[::3]
    with pytest.raises(NotImplementedError):
        cp.select_tracklets(dict(selection=dict(mode='longest', size=1.0)), items)


def test_frame_indices_and_strict_increase():
    a = Tracklet(torch.zeros(3, 7), [30, 50, 90])
    b = Tracklet(torch.zeros(2, 7), [10, 50])
    ts2frame = cp.segment_ts2frame([a], [b])
    assert ts2frame == {10: 0, 30: 1, 50: 2, 90: 3}
    assert cp.frame_indices(a.ts_list, ts2frame) == [1, 2, 3] and cp.frame_indices(b.ts_list, ts2frame) == [0, 2]
    with pytest.raises(ValueError):
        cp.frame_indices([50, 30], ts2frame)
    with pytest.raises(ValueError):
        cp.frame_indices([50, 50], ts2frame)
    boxes, offsets, frames = cp.pack_tracklets([a, b], ts2frame)
    assert boxes.shape == (5, 7) and offsets.tolist() == [0, 3, 5] and frames.tolist() == [1, 2, 3, 0, 2]
    assert offsets.dtype == frames.dtype == torch.int32


def test_enlarged_boxes():
    b = torch.tensor([[1., 2., 3., 2., 4., 1.5, 0.3], [0., 0., 0., 0.5, 4., 1.5, -1.]])
    e = cp.enlarged_boxes(b, 1)
    assert torch.equal(e[0], torch.tensor([1., 2., 2., 4., 6., 3.5, 0.3])) and torch.equal(b[0, 2], torch.tensor(3.))
    s = cp.enlarged_boxes(b, -0.25)
    assert torch.allclose(s[0], torch.tensor([1., 2., 3.25, 1.5, 3.5, 1.0, 0.3]))
    assert torch.equal(s[1], b[1])      # would turn inside out: kept


def test_cpu_tensors_raise():
    with pytest.raises(L.OcoccError):
        cp.crop_frames([torch.zeros(4, 6)], [torch.zeros(1, 7)])
    with pytest.raises(L.OcoccError):
        cp.crop_frames_packed(torch.zeros(4, 6), [0, 4], torch.zeros(1, 7), [0, 1])
    t = Tracklet(torch.zeros(2, 7), [1, 2])
    with pytest.raises(L.OcoccError):
        cp.tracklet_max_iou([t], [t])
    z = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(L.OcoccError):
        cp.max_iou_packed(torch.zeros(2, 7), z, z, torch.zeros(2, 7), z, z)


def test_more_than_sixteen_processes_refused(tmp_path):
    with pytest.raises(ValueError, match='16'):
        cp.generate_track_input(dict(name='x', split='training'), process=17)
    with pytest.raises(ValueError, match='16'):
        cp.generate_candidates(dict(name='x', split='training'), process=17)
    for tool in ('generate_track_input.py', 'generate_candidates.py'):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'ctrl', tool), str(tmp_path / 'none.yaml'), '--process', '17'],
                           capture_output=True, text=True)
        assert r.returncode == 2 and '--process 17' in r.stderr and '16' in r.stderr


def test_new_exports_declared_with_signatures():
    src = open(os.path.join(ROOT, 'include', 'ococc_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(ococc_[a-z0-9_]+)\s*\(', src))
    for name in ('ococc_tracklet_crop_count', 'ococc_tracklet_crop_fill', 'ococc_tracklet_max_iou_f32'):
        assert name in declared and name in L.SIGNATURES and hasattr(L.lib, name)
    assert set(declared) <= set(L.SIGNATURES)


def test_files_round_trip_through_the_dataset(tmp_path, monkeypatch):
    """raw tree -> track input -> candidates on the CPU stand-ins -> WaymoTrackletDatasetWithOcc reads all three"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_synthetic_raw
    from objectcentricocccompletion_amd import waymo_io
    from objectcentricocccompletion_amd.dataset import WaymoTrackletDatasetWithOcc
    raw = str(tmp_path / 'raw')
    make_synthetic_raw.main([raw, '--segments', '2', '--tracklets', '2', '--frames', '34', '--background', '400'])
    config = os.path.join(raw, 'synthetic_vehicle.yaml')
    monkeypatch.setattr(cp, 'crop_frames_packed', crop_packed_f64)
    monkeypatch.setattr(cp, 'max_iou_packed', max_iou_packed_oracle)
    monkeypatch.setattr(cp, 'CROP_BATCH_BYTES', 200_000)      # several batches per segment
    info = cp.generate_track_input(config, device='cpu')
    cand = cp.generate_candidates(config, os.path.join(raw, 'waymo_format', 'train_gt.bin'), device='cpu')
    assert info == os.path.join(raw, 'tracklet_data', 'synthetic_vehicle_training.pkl')
    assert cand == os.path.join(raw, 'tracklet_data', 'synthetic_vehicle_training_gt_candidates.pkl')
    infos, cands = pickle.load(open(info, 'rb')), pickle.load(open(cand, 'rb'))
    detections = waymo_io.generate_tracklets(waymo_io.read_bin(os.path.join(raw, 'waymo_format', 'pred.bin')))
    assert [(e[0], e[1]) for e in infos] == [(t.segment_name, t.id) for t in detections] and len(cands) == len(infos) == 6
    for e, c in zip(infos, cands):
        seg, tid, type_, in_world, boxes, ts, scores, num_pts = e
        assert type_ == 1 and in_world is False and boxes[0].shape == (1, 7) and len(boxes) == len(ts) == len(scores) == len(num_pts)
        pts = np.load(os.path.join(raw, 'tracklet_data', 'synthetic_vehicle_training_database', f'{seg}--{tid}.npy'), allow_pickle=True)
        assert len(pts) == len(ts) and [len(p) for p in pts] == num_pts
        assert all(p.dtype == np.float32 and p.ndim == 2 and p.shape[1] == 6 for p in pts)
        # every frame's rows are the cloud's rows inside the enlarged box, in the cloud's order
        k = len(ts) // 2
        idx2ts = pickle.load(open(os.path.join(raw, 'kitti_format', 'idx2timestamp.pkl'), 'rb'))
        idx = {v: i for i, v in idx2ts.items()}[ts[k]]
        cloud = np.fromfile(os.path.join(raw, 'kitti_format', 'training', 'velodyne', idx + '.bin'), np.float32).reshape(-1, 6)
        big = cp.enlarged_boxes(torch.from_numpy(boxes[k]), 1).numpy()[0]
        assert np.array_equal(pts[k], cloud[in_box_f64(cloud[:, :3], big)])
        if tid.endswith('_fp'):
            assert c == [] and sum(num_pts) < 100
        else:
            assert [g[1] for g in c] == [tid.replace('trk', 'gt')] and c[0][0] == seg and c[0][7] is None
    with pytest.raises(FileExistsError):
        cp.generate_track_input(dict(cp.load_config(config)[0], name='synthetic_vehicle', exist_ok=False), device='cpu')
    j = lambda p: os.path.join(raw, p)
    ds = WaymoTrackletDatasetWithOcc(raw, cand, info, j('occ_gt'), j('poses.pkl'), pipeline=None, classes=['Car'],
                                     min_tracklet_points=100, min_tracklet_length=32)
    assert len(ds) == 4                                          # the two false positives hold too few points
    for i in range(len(ds)):
        d = ds.get_data_info(i)
        assert os.path.isfile(d['pts_filename']) and len(d['ann_info']) == 1
        assert all(os.path.isfile(o['occ_label_name']) for o in d['occ_infos'])
