"""CPU suite: the native Waymo detection metric (objectcentricocccompletion_amd/waymo_metrics.py) -- the new proto fields
against the protobuf library, level assignment, the float64 checker (tests/waymo_metrics_ref.py) on closed-form cases and
hand-built scenes, the text round trip, and the refusal to run without a device.  The kernels themselves are checked
against the same checker in tests/test_gpu_waymo_metrics.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import waymo_metrics_ref as R   # noqa: E402

from objectcentricocccompletion_amd import waymo_io as W   # noqa: E402
from objectcentricocccompletion_amd.tracklet import Tracklet   # noqa: E402


# ------------------------------------------------------------------------------------------------ proto fields
def _schema():
    """The schema of tests/test_waymo_io_cpu.py plus Label.detection_difficulty_level = 5 and
    Label.num_lidar_points_in_box = 7 (published label.proto), in google.protobuf's descriptor pool"""
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    fd = descriptor_pb2.FileDescriptorProto()
    fd.name, fd.package, fd.syntax = 'ococc_test_waymo_metrics.proto', 'ococc_test_waymo_metrics', 'proto2'
    D = descriptor_pb2.FieldDescriptorProto
    label = fd.message_type.add()
    label.name = 'Label'
    box = label.nested_type.add()
    box.name = 'Box'
    for i, n in enumerate(['center_x', 'center_y', 'center_z', 'width', 'length', 'height', 'heading'], 1):
        f = box.field.add()
        f.name, f.number, f.label, f.type = n, i, D.LABEL_OPTIONAL, D.TYPE_DOUBLE
    f = label.field.add()
    f.name, f.number, f.label, f.type, f.type_name = 'box', 1, D.LABEL_OPTIONAL, D.TYPE_MESSAGE, '.ococc_test_waymo_metrics.Label.Box'
    for n, num, t in (('type', 3, D.TYPE_INT32), ('id', 4, D.TYPE_STRING), ('detection_difficulty_level', 5, D.TYPE_INT32),
                      ('num_lidar_points_in_box', 7, D.TYPE_INT32)):     # (an enum on the wire is a varint)
        f = label.field.add()
        f.name, f.number, f.label, f.type = n, num, D.LABEL_OPTIONAL, t
    obj = fd.message_type.add()
    obj.name = 'Object'
    for n, num, t, tn in (('object', 1, D.TYPE_MESSAGE, '.ococc_test_waymo_metrics.Label'), ('score', 2, D.TYPE_FLOAT, None),
                          ('overlap_with_nlz', 3, D.TYPE_BOOL, None), ('context_name', 4, D.TYPE_STRING, None),
                          ('frame_timestamp_micros', 5, D.TYPE_INT64, None)):
        f = obj.field.add()
        f.name, f.number, f.label, f.type = n, num, D.LABEL_OPTIONAL, t
        if tn:
            f.type_name = tn
    objs = fd.message_type.add()
    objs.name = 'Objects'
    f = objs.field.add()
    f.name, f.number, f.label, f.type, f.type_name = 'objects', 1, D.LABEL_REPEATED, D.TYPE_MESSAGE, '.ococc_test_waymo_metrics.Object'
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    get = getattr(message_factory, 'GetMessageClass', None)
    if get is None:
        get = message_factory.MessageFactory(pool).GetPrototype
    return get(pool.FindMessageTypeByName('ococc_test_waymo_metrics.Objects'))


def _tracklets():
    g = torch.Generator().manual_seed(5)
    out = []
    for t in range(2):
        n = 5 + t
        b = torch.rand(n, 7, generator=g) * 4 + 1
        out.append(Tracklet(b, [1550000000000000 + 100000 * i for i in range(n)], torch.rand(n, generator=g), type=[0, 2][t],
                            segment_name=f'segment-{t:03d}', id=f'obj_{t}'))
    return out


def test_new_fields_equal_the_protobuf_library_and_defaults_keep_the_bytes(tmp_path):
    Objects = _schema()
    trks = _tracklets()
    nlz = [[i % 2 == 0 for i in range(len(t))] for t in trks]
    lvl = [[i % 3 for i in range(len(t))] for t in trks]
    pts = [[0, 3, 5, 6, 1000, 70000, 2 ** 31 - 1][:len(t)] for t in trks]
    path = W.convert_tracklet_to_waymo(trks, str(tmp_path / 'full'), overlap_with_nlz=nlz, detection_difficulty_level=lvl,
                                       num_lidar_points_in_box=pts)
    plain = W.convert_tracklet_to_waymo(trks, str(tmp_path / 'plain'))
    ref_full, ref_plain = Objects(), Objects()
    classes = ('Car', 'Pedestrian', 'Cyclist')
    for k, trk in enumerate(trks):
        for i in range(len(trk)):
            plain_obj = Objects.FromString(W._f_bytes(1, W.lidar2waymo_box(
                trk.boxes[i].numpy(), trk.scores[i].item(), W.K2W_CLS_MAP[classes[trk.type]], trk.segment_name, trk.ts_list[i],
                trk.id))).objects[0]
            ref_plain.objects.add().CopyFrom(plain_obj)
            o = ref_full.objects.add()
            o.CopyFrom(plain_obj)
            o.overlap_with_nlz = nlz[k][i]
            o.object.detection_difficulty_level = lvl[k][i]
            o.object.num_lidar_points_in_box = pts[k][i]
    assert open(path, 'rb').read() == ref_full.SerializeToString()
    # defaults: the bytes of the writer as it was (the library's serialisation of the same objects without the fields)
    assert open(plain, 'rb').read() == ref_plain.SerializeToString()
    assert len(open(path, 'rb').read()) > len(open(plain, 'rb').read())
    recs = W.read_bin(path)
    for r, o in zip(recs, ref_full.objects):
        assert r['overlap_with_nlz'] is bool(o.overlap_with_nlz)
        assert r['detection_difficulty_level'] == o.object.detection_difficulty_level
        assert r['num_lidar_points_in_box'] == o.object.num_lidar_points_in_box
    for r in W.read_bin(plain):     # absent fields read as False / 0
        assert r['overlap_with_nlz'] is False and r['detection_difficulty_level'] == 0 and r['num_lidar_points_in_box'] == 0
    # a negative int32 is ten bytes on the wire and reads back negative
    one = W.lidar2waymo_box(np.ones(7), 0.5, 1, 'c', 1, 'x', num_lidar_points_in_box=-2)
    m = Objects.FromString(W._f_bytes(1, one)).objects[0]
    assert m.object.num_lidar_points_in_box == -2


# ------------------------------------------------------------------------------------------------ levels
def test_level_assignment():
    from objectcentricocccompletion_amd.waymo_metrics import IGNORED, LEVEL_1, LEVEL_2, gt_levels
    diff = np.array([0, 0, 0, 0, 0, 1, 1, 2, 2, 1])
    pts = np.array([0, 1, 5, 6, 900, 0, 3, 0, 100, 100])
    exp = [IGNORED, LEVEL_2, LEVEL_2, LEVEL_1, LEVEL_1, IGNORED, LEVEL_2, LEVEL_2, LEVEL_2, LEVEL_1]
    assert gt_levels(diff, pts).tolist() == exp
    exp_assume = [LEVEL_1, LEVEL_2, LEVEL_2, LEVEL_1, LEVEL_1, LEVEL_1, LEVEL_2, LEVEL_2, LEVEL_2, LEVEL_1]
    assert gt_levels(diff, pts, assume_points=True).tolist() == exp_assume
    for d, n, e, ea in zip(diff, pts, exp, exp_assume):      # the checker states the same rule on its own
        o = dict(detection_difficulty_level=int(d), num_lidar_points_in_box=int(n))
        assert R.gt_level(o) == e and R.gt_level(o, True) == ea


# ------------------------------------------------------------------------------------------------ the checker itself
def test_checker_iou_closed_forms():
    far = [70.0, -60.0, 1.0]
    a = far + [4.5, 2.0, 1.6, 0.7]
    assert R.iou3d(a, a) == pytest.approx(1.0, abs=1e-12)
    # axis-aligned half shift: intersection 1/2 of either, union 3/2
    assert R.iou3d([0, 0, 0, 2, 2, 2, 0], [1, 0, 0, 2, 2, 2, 0]) == pytest.approx(1 / 3, abs=1e-12)
    assert R.iou3d([0, 0, 0, 2, 2, 2, 0], [0, 0, 1, 2, 2, 2, 0]) == pytest.approx(1 / 3, abs=1e-12)
    # a unit square turned 45 degrees lies inside the 4 x 4 one: 1 / 16
    assert R.iou3d([5, 5, 0, 1, 1, 1, math.pi / 4], [5, 5, 0, 4, 4, 1, 0]) == pytest.approx(1 / 16, abs=1e-12)
    # ... and turned 45 degrees inside a 1.2 x 1.2 one its corners are cut: area 1 - 4 * (sqrt(.5) - .6)^2
    cut = 1 - 4 * (math.sqrt(0.5) - 0.6) ** 2
    assert R.iou3d([5, 5, 0, 1, 1, 1, math.pi / 4], [5, 5, 0, 1.2, 1.2, 1, 0]) == pytest.approx(cut / (1 + 1.44 - cut), abs=1e-12)
    assert R.iou3d([0, 0, 0, 2, 2, 2, 0], [2, 0, 0, 2, 2, 2, 0]) == 0.0          # touching
    assert R.iou3d([0, 0, 0, 2, 2, 2, 0], [0, 0, 2, 2, 2, 2, 0]) == 0.0          # touching in height
    assert R.iou3d([0, 0, 0, 2, 2, 2, 0], [10, 0, 0, 2, 2, 2, 1.0]) == 0.0       # disjoint
    assert R.iou3d([0, 0, 0, 0, 2, 2, 0], [0, 0, 0, 2, 2, 2, 0]) == 0.0          # zero extent
    assert R.iou3d([float('nan'), 0, 0, 2, 2, 2, 0], [0, 0, 0, 2, 2, 2, 0]) == 0.0


def _scene():
    """3 frames x 2 vehicles, all LEVEL_1, near the origin; predictions = ground truth, scores 0.9 .. 0.4"""
    gts, preds = [], []
    for f in range(3):
        for k in range(2):
            box = [5.0 + 10 * k, 2.0 * f, 1.0, 4.5, 2.0, 1.6, 0.3 + 0.1 * k]
            gts.append(R.make_object(box, 1, 1.0, 'seg', f, points=50))
            preds.append(R.make_object(box, 1, 0.9 - 0.1 * (2 * f + k), 'seg', f))
    return preds, gts


def test_checker_scenes_with_known_answers():
    preds, gts = _scene()
    tab, ap = R.detection_metrics(preds, gts)
    assert R.match(preds, gts) == list(range(6))
    assert ap['Vehicle/L1 mAP'] == pytest.approx(1.0, abs=1e-12) and ap['Vehicle/L1 mAPH'] == pytest.approx(1.0, abs=1e-12)
    assert ap['Vehicle/L2 mAP'] == pytest.approx(1.0, abs=1e-12) and ap['Pedestrian/L1 mAP'] == 0.0
    assert tab['RANGE_TYPE_VEHICLE_[0, 30)_LEVEL_1'][0] == pytest.approx(1.0, abs=1e-12)
    assert tab['RANGE_TYPE_VEHICLE_[30, 50)_LEVEL_1'] == (0.0, 0.0)       # no ground truth there
    # all headings off by pi: every pair still matches (the rectangle is the same), heading accuracy 0
    flipped = [dict(p, heading=p['heading'] + math.pi) for p in preds]
    _, ap = R.detection_metrics(flipped, gts)
    assert ap['Vehicle/L1 mAP'] == pytest.approx(1.0, abs=1e-9) and ap['Vehicle/L1 mAPH'] == pytest.approx(0.0, abs=1e-9)
    # one false positive scored above everything (0.95): at every cutoff that keeps a true positive the false positive is
    # kept too, so with k true positives precision is k / (k + 1) and recall k / 6.  Cutoffs 0 .. 0.4 keep all six
    # (6/7 at recall 1), then 0.41-0.5 five (5/6), ... 0.81-0.9 one (1/2), 0.91-0.95 none (precision 0 at recall 0).
    # Made non-increasing from the right, every recall step k/6 carries max over k' >= k of k'/(k'+1) = 6/7:
    # AP = 6 * (1/6) * 6/7 = 6/7.
    fp = R.make_object([40.0, 40.0, 1.0, 4.5, 2.0, 1.6, 0.0], 1, 0.95, 'seg', 0)
    tab, ap = R.detection_metrics(preds + [fp], gts)
    assert ap['Vehicle/L1 mAP'] == pytest.approx(6 / 7, abs=1e-12) and ap['Vehicle/L1 mAPH'] == pytest.approx(6 / 7, abs=1e-12)
    assert tab['RANGE_TYPE_VEHICLE_[0, 30)_LEVEL_1'][0] == pytest.approx(1.0, abs=1e-12)    # the false positive sits at 56 m
    assert tab['RANGE_TYPE_VEHICLE_[50, +inf)_LEVEL_1'] == (0.0, 0.0)                       # ... where no ground truth is
    # a prediction on an L2 object is neither a true nor a false positive in LEVEL_1
    gts2 = [dict(g) for g in gts]
    gts2[0]['num_lidar_points_in_box'] = 3          # LEVEL_2 by its point count; its prediction has the top score
    _, ap = R.detection_metrics(preds, gts2)
    assert ap['Vehicle/L1 mAP'] == pytest.approx(1.0, abs=1e-12)      # 5 L1 objects, 5 true positives, no false positive
    assert ap['Vehicle/L2 mAP'] == pytest.approx(1.0, abs=1e-12)
    # an ignored object cannot be matched: its prediction becomes a false positive (the top-scored one: 5/6 by the
    # argument above with five true positives)
    gts2[0]['num_lidar_points_in_box'] = 0
    _, ap = R.detection_metrics(preds, gts2)
    assert ap['Vehicle/L1 mAP'] == pytest.approx(5 / 6, abs=1e-12)
    # NLZ predictions are dropped
    _, ap = R.detection_metrics(preds + [dict(fp, overlap_with_nlz=True)], gts)
    assert ap['Vehicle/L1 mAP'] == pytest.approx(1.0, abs=1e-12)


def test_host_curves_equal_the_checker_given_the_checkers_matches():
    """waymo_metrics.pack / curves (numpy, what runs after the kernels) against the checker's loops, the match indices taken
    from the checker and mapped into packed order"""
    from objectcentricocccompletion_amd import waymo_metrics as M
    rng = np.random.default_rng(11)
    preds, gts, _, _ = R.decisive_frames(rng, [(int(rng.integers(0, 25)), int(rng.integers(0, 20))) for _ in range(25)])
    preds = [preds[i] for i in rng.permutation(len(preds))]
    gts = [gts[i] for i in rng.permutation(len(gts))]
    m = R.match(preds, gts)
    pk = M.pack(M.columns(preds), M.columns(gts))
    inv = np.empty(len(gts), dtype=np.int64)
    inv[pk['gt_order']] = np.arange(len(gts))
    packed = np.array([inv[m[i]] if m[i] >= 0 else -1 for i in pk['pd_order']])
    got = M.curves(pk, packed)
    exp = R.table(preds, gts, m)
    assert list(got) == list(exp)
    assert sum(1 for v in exp.values() if v[0] > 0) >= 16
    for k in exp:
        assert got[k] == pytest.approx(exp[k], abs=1e-12), k
    # predictions are sorted by (frame, type, descending score), ground truth grouped by frame
    for f in range(pk['F']):
        a, b = pk['pd_offsets'][f], pk['pd_offsets'][f + 1]
        key = list(zip(pk['pd_type'][a:b], -pk['pd_score'][a:b]))
        assert key == sorted(key)


def test_text_round_trips_through_parse_detection_metrics():
    from objectcentricocccompletion_amd import waymo_metrics as M
    preds, gts = _scene()
    tab = R.table(preds + [R.make_object([40.0, 40.0, 1.0, 4.5, 2.0, 1.6, 0.0], 1, 0.95, 'seg', 0)], gts, list(range(6)) + [-1])
    text = M.HEADER + M.format_table(tab)
    lines = [l for l in text.splitlines() if not l.startswith('#')]
    assert lines[0].startswith('OBJECT_TYPE_TYPE_VEHICLE_LEVEL_1: [mAP 0.857142857142857] [mAPH ')
    assert lines[8].startswith('RANGE_TYPE_VEHICLE_[0, 30)_LEVEL_1: [mAP 1] [mAPH 1]') and len(lines) == 32
    assert lines[-1] == 'RANGE_TYPE_CYCLIST_[50, +inf)_LEVEL_2: [mAP 0] [mAPH 0]'
    assert 'Hungarian' in M.HEADER and 'recall-delta' in M.HEADER and 'not been measured' in M.HEADER
    ap = W.parse_detection_metrics(text)
    exp = R.ap_dict(tab)
    assert set(ap) == set(exp)
    for k in exp:
        assert ap[k] == pytest.approx(exp[k], abs=1e-12)
    assert ap['Overall/L1 mAP'] == pytest.approx((6 / 7) / 3, abs=1e-12)


# ------------------------------------------------------------------------------------------------ public interface
def _dataset(tmp_path):
    from objectcentricocccompletion_amd.dataset import WaymoTrackletDatasetWithOcc
    ds = WaymoTrackletDatasetWithOcc.__new__(WaymoTrackletDatasetWithOcc)
    ds.CLASSES = ('Car',)
    ds.data_root = str(tmp_path / 'kitti_format') + '/'
    return ds


def test_unknown_metric_still_raises_keyerror_and_names_waymo_native(tmp_path):
    ds = _dataset(tmp_path)
    with pytest.raises(KeyError, match='waymo_native'):
        ds.evaluate([], metric='bbox')
    with pytest.raises(KeyError):
        ds.evaluate([], metric=['iou', 'bbox'])


def test_waymo_native_refuses_to_run_without_a_device(tmp_path, monkeypatch):
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd import waymo_metrics as M
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    with pytest.raises(L.OcoccError):       # CPU tensors
        M.frame_match(z(1, 7), z(1, dt=torch.int32), z(1, dt=torch.int32), [0, 1], z(1, 7), z(1, dt=torch.int32),
                      z(1, dt=torch.int32), [0, 1])
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)     # (so that the test says the same on a GPU machine)
    preds, gts = _scene()
    with pytest.raises(L.OcoccError):
        M.detection_metrics(preds, gts)
    # through the dataset: the .bin is written, then the same error
    ds = _dataset(tmp_path)
    os.makedirs(tmp_path / 'waymo_format')
    trk = Tracklet(torch.ones(2, 7), [10, 11], segment_name='segment-000', id='a')
    W.convert_tracklet_to_waymo([trk], str(tmp_path / 'waymo_format' / 'gt.bin'))
    with pytest.raises(L.OcoccError):
        ds.evaluate([dict(out_tracklets=[trk])], metric='waymo_native', pklfile_prefix=str(tmp_path / 'result_val'))
    assert os.path.isfile(tmp_path / 'result_val.bin')


def test_frame_match_abi_argument_errors():
    """the export's checks run before anything touches a device"""
    from objectcentricocccompletion_amd import _lib as L
    thr = (L.c_f32 * 5)(0, .7, .5, .5, .5)
    assert L.lib.ococc_frame_match_workspace_bytes(1000) >= 4000 and L.lib.ococc_frame_match_workspace_bytes(-1) == -1
    call = lambda max_gt, thr, ws: L.lib.ococc_frame_match_f32(None, None, None, None, 0, None, None, None, None, 0, None, 0, 0,
                                                               0, 100, max_gt, thr, None, None, None, ws, None)
    assert call(5000, thr, 1 << 20) == -1 and b'4096' in L.lib.ococc_last_error()
    assert call(10, (L.c_f32 * 5)(0, 0, .5, .5, .5), 1 << 20) == -1 and b'thresholds' in L.lib.ococc_last_error()
    assert call(10, thr, 16) == -1 and b'workspace' in L.lib.ococc_last_error()
    assert call(10, thr, 1 << 20) == 0          # no frames: nothing to launch


def test_synthetic_dataset_writes_a_ground_truth_file_with_all_levels(tmp_path):
    import subprocess
    root = str(tmp_path / 'data')
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'make_synthetic_dataset.py')
    subprocess.run([sys.executable, tool, root, '--tracklets', '2', '--frames', '20'], check=True, capture_output=True, timeout=300)
    objs = W.read_bin(os.path.join(root, 'waymo_format', 'gt.bin'))
    assert len(objs) == 40 and {o['type'] for o in objs} == {1}
    assert sorted({R.gt_level(o) for o in objs}) == [0, 1, 2]
    assert sum(R.gt_level(o) == 2 for o in objs) == 8 and sum(R.gt_level(o) == 0 for o in objs) == 4
