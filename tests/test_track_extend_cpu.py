"""Track extension and empty-box removal (objectcentricocccompletion_amd/ctrl_prep.py, tools/ctrl/extend_tracks.py,
tools/ctrl/remove_empty.py), the part that needs no GPU: the host plan against the reference golden
(tests/golden/track_extend.npz, tools/gen_golden_track_extend.py), configuration, the record writer, argument errors,
the export table, and the two tools on the synthetic raw tree with the device operators replaced by float64
restatements."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from objectcentricocccompletion_amd import _lib as L  # noqa: E402
from objectcentricocccompletion_amd import ctrl_prep as cp  # noqa: E402
from objectcentricocccompletion_amd import waymo_io  # noqa: E402
from test_gpu_track_extend import CASES, extend_f64, load_fixture  # noqa: E402  (restatement and fixture loader; no GPU at import)

NEW_EXPORTS = ('ococc_track_extend_f64', 'ococc_tracklet_nonempty')

REFERENCE_SHAPED_YAML = """\
bin_path: /somewhere/tracker_output.bin
direction: backward # only backward here
extend_length: 10
min_length_to_extend: 3
score_multiplier: 0.01
velo_window_size: 10
"""


def seg_lists(fx):
    return [[int(v) for v in fx['timestamps'][a:b]] for a, b in zip(fx['seg_offsets'], fx['seg_offsets'][1:])]


@pytest.mark.parametrize('case', CASES)
def test_host_plan_equals_reference_golden(case):
    fx, cfgs = load_fixture()
    cfg = cfgs[case]
    back, fwd, out_offsets = cp.plan_extension(fx['offsets'], fx['frames'], fx['segments'], seg_lists(fx), cfg['extend_length'],
                                               cfg['min_length'], cfg['extend_all'], cfg['min_length_all'])
    assert out_offsets.dtype == back.dtype == fwd.dtype == np.int32
    assert np.array_equal(out_offsets, fx[f'{case}_out_offsets'])                  # who extends, and L'
    lens = np.diff(fx['offsets'])
    assert np.array_equal(np.diff(out_offsets), lens + back + fwd)
    stamps = []                                                                    # the output timestamps
    for t, s in enumerate(fx['segments']):
        ts = seg_lists(fx)[s]
        fr = fx['frames'][fx['offsets'][t]:fx['offsets'][t + 1]]
        stamps += ts[fr[0] - back[t]:fr[0]] + [ts[f] for f in fr] + ts[fr[-1] + 1:fr[-1] + 1 + fwd[t]]
    assert np.array_equal(np.asarray(stamps), fx[f'{case}_out_timestamps'])
    # the branches of the catalogue (two segments of 20 tracklets, the same frames in both)
    per_seg = len(lens) // 2
    b, f = back.reshape(2, per_seg), fwd.reshape(2, per_seg)
    assert b[:, 0].tolist() == [0, 0] and b[:, 1].tolist() == [0, 0] and b[:, 2].tolist() == [0, 0]     # short, single, frame 0
    assert b[0, 8] > 0 and b[1, 8] == 0 and f[1, 8] == 0        # first gap 500 000 (regular segment) / 500 001 us
    assert b[0, 9] > 0 and b[1, 9] > 0                          # first gap exactly 500 000 us in both
    if case == 'extend':
        assert (fwd == 0).all() and b[:, 3].tolist() == [3, 3] and b[:, 4].tolist() == [10, 10] and b[:, 13].tolist() == [2, 2]
    else:
        assert b[:, 7].tolist() == [14, 14] and f[:, 7].tolist() == [10, 10] and f[:, 6].tolist() == [0, 0] and b[:, 6].tolist() == [22, 22]
        assert b[:, 11].tolist() == [10, 10] and f[:, 11].tolist() == [0, 0]      # exactly min_length_to_extend_all: plain extend
        assert b[:, 12].tolist() == [11, 11] and f[:, 12].tolist() == [42, 42]    # one more box: extend_all
        assert b[:, 3].tolist() == [3, 3] and f[:, 3].tolist() == [40, 40]


def test_golden_margin_and_restatement():
    """the stored margin is what the restatement and the golden differ by on this machine too (within the factor the
    GPU test allows for another platform's float32 inverse), and stays below the 5 cm alarm"""
    fx, cfgs = load_fixture()
    from test_gpu_track_extend import wrapped
    assert 0 < float(fx['margin']) <= 0.05
    for case in CASES:
        exp = np.concatenate([e[0] for e in extend_f64(fx, cfgs[case])], 0)
        d = np.abs(wrapped(exp - fx[f'{case}_out_boxes'].astype(np.float64)))
        assert d.max() <= 2 * float(fx['margin'])
        es = np.concatenate([e[1] for e in extend_f64(fx, cfgs[case])])
        assert np.allclose(es, fx[f'{case}_out_scores'], rtol=1e-14, atol=0)
    assert np.abs(fx['poses'].reshape(-1, 4, 4)[:, :3, 3]).max() > 3000        # kilometres from the origin


def test_plan_rules_directly():
    seg_ts = [[0, 100_000, 200_000, 700_000, 800_000, 900_000, 1_400_001, 1_500_000]]
    plan = lambda frames, **kw: cp.plan_extension([0, len(frames)], frames, [0], seg_ts, **{**dict(extend_length=10, min_length=3), **kw})
    assert [v.tolist() for v in plan([3, 4, 5])] == [[3], [0], [0, 6]]
    assert [v.tolist() for v in plan([3, 4, 5], extend_length=2)] == [[2], [0], [0, 5]]
    assert [v.tolist() for v in plan([2, 3, 4])] == [[2], [0], [0, 5]]                    # gap of exactly 500 000
    assert [v.tolist() for v in plan([5, 6, 7])] == [[0], [0], [0, 3]]                    # gap of 500 001
    assert [v.tolist() for v in plan([3, 4])] == [[0], [0], [0, 2]]                       # shorter than min_length
    assert [v.tolist() for v in plan([4], min_length=1)] == [[0], [0], [0, 1]]            # one box: never extended
    assert [v.tolist() for v in plan([3, 4, 5], extend_all=True, min_length_all=2)] == [[3], [2], [0, 8]]
    assert [v.tolist() for v in plan([3, 4, 5], extend_all=True, min_length_all=3)] == [[3], [0], [0, 6]]   # L > min, not >=
    assert [v.tolist() for v in plan([5, 6, 7], extend_all=True, min_length_all=2)] == [[0], [0], [0, 3]]   # the gap cancels both
    with pytest.raises(NotImplementedError):
        plan([3, 4, 5], direction='forward')


def test_extend_config(tmp_path):
    path = tmp_path / 'extend.yaml'
    path.write_text(REFERENCE_SHAPED_YAML)
    cfg, name = cp.load_extend_config(str(path))
    assert name == 'extend' and cfg['extend_length'] == 10 and cfg['score_multiplier'] == 0.01 and cfg['direction'] == 'backward'
    shipped, shipped_name = cp.load_extend_config(os.path.join(ROOT, 'tools', 'ctrl', 'data_configs', 'synthetic_extend.yaml'))
    assert set(cfg) <= set(shipped) and shipped_name == 'synthetic_extend'
    with pytest.raises(NotImplementedError):
        cp.load_extend_config(dict(cfg, name='x', direction='forward'))
    with pytest.raises(ValueError):
        cp.load_extend_config(dict(cfg, name='x', direction='sideways'))
    with pytest.raises(KeyError):
        cp.load_extend_config({k: v for k, v in cfg.items() if k != 'velo_window_size'} | dict(name='x'))
    with pytest.raises(KeyError):
        cp.load_extend_config(dict(cfg, name='x', extend_all=True))
    with pytest.raises(KeyError):
        cp.load_extend_config(cfg)                      # a mapping needs a name


def test_write_objects_round_trip(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_synthetic_raw
    raw = str(tmp_path / 'raw')
    make_synthetic_raw.main([raw, '--segments', '1', '--tracklets', '2', '--frames', '12', '--background', '50'])
    for name in ('pred.bin', 'gt.bin'):
        src = os.path.join(raw, 'waymo_format', name)
        recs = waymo_io.read_bin(src)
        out = waymo_io.write_objects(recs, str(tmp_path / name))
        assert waymo_io.read_bin(out) == recs and len(recs) > 10
    assert open(tmp_path / 'pred.bin', 'rb').read() == open(os.path.join(raw, 'waymo_format', 'pred.bin'), 'rb').read()
    rec = dict(waymo_io.read_bin(os.path.join(raw, 'waymo_format', 'gt.bin'))[0], overlap_with_nlz=True, num_lidar_points_in_box=-3,
               frame_timestamp_micros=-5, score=0.1)
    got = waymo_io.read_bin(waymo_io.write_objects([rec], str(tmp_path / 'one.bin')))
    assert got == [dict(rec, score=float(np.float32(0.1)))]              # the score is a 32-bit float on the wire
    assert waymo_io.read_bin(waymo_io.write_objects([], str(tmp_path / 'none.bin'))) == []


def test_lifted_boxes():
    rec = dict(center_x=1.0, center_y=2.0, center_z=3.0, width=2.0, length=4.5, height=1.5, heading=0.25)
    b = cp.lifted_lidar_boxes([rec, dict(rec, heading=3.0)], 0.2)
    assert b.dtype == torch.float32 and b.shape == (2, 7)
    assert torch.allclose(b[0], torch.tensor([1.0, 2.0, 3.0 - 0.75 + 0.3, 2.0, 4.5, 1.5, -0.25 - np.pi / 2]))
    assert abs(float(b[1, 6]) - (-3.0 - np.pi / 2 + 2 * np.pi)) < 1e-6       # wrapped into [-pi, pi]
    assert cp.lifted_lidar_boxes([], 0.2).shape == (0, 7)


def test_argument_errors():
    z = torch.zeros
    with pytest.raises(L.OcoccError):
        cp.nonempty_frames_packed(z(4, 6), [0, 4], z(1, 7), [0, 1])
    with pytest.raises(L.OcoccError):
        cp.extend_tracks_packed(z(2, 7), [0, 2], [0, 1], [0], z(2, dtype=torch.float64), z(2, 16), z(2, dtype=torch.int64), [0, 2],
                                [0], [0], [0, 2], 0.9, 10)
    if not torch.cuda.is_available():                      # no CPU fallback: refused before any file is read
        with pytest.raises(L.OcoccError, match='ROCm'):
            cp.extend_tracks(dict(name='x', bin_path='a.bin', direction='backward', extend_length=1, min_length_to_extend=3,
                                  score_multiplier=0.9, velo_window_size=10))
    with pytest.raises(ValueError, match='16'):
        cp.remove_empty('a.bin', 'training', process=17)
    with pytest.raises(NotImplementedError):
        cp.remove_empty('a.bin', 'training', type='sign')
    with pytest.raises(ValueError):
        cp.remove_empty('a.bin', 'train')
    with pytest.raises(NotImplementedError):
        cp.remove_empty('a.bin', 'training', extra_hw=0.1)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'ctrl', 'remove_empty.py'), '--bin-path', 'none.bin', '--process', '17'],
                       capture_output=True, text=True)
    assert r.returncode == 2 and '--process 17' in r.stderr and '16' in r.stderr
    # the C entry points report argument errors
    rc = L.lib.ococc_track_extend_f64(None, None, None, None, None, 1, 1, None, None, None, 1, 1, None, None, None, 1, 0.9, 10,
                                      None, None, None, None)
    assert rc == -1 and b'null pointer' in L.lib.ococc_last_error()
    rc = L.lib.ococc_track_extend_f64(None, None, None, None, None, 1, 2, None, None, None, 1, 1, None, None, None, 1, 0.9, 10,
                                      None, None, None, None)
    assert rc == -1 and b'num_out' in L.lib.ococc_last_error()
    rc = L.lib.ococc_track_extend_f64(None, None, None, None, None, 1, 1, None, None, None, 1, 1, None, None, None, 1, 0.9, 0,
                                      None, None, None, None)
    assert rc == -1 and b'velo_window_size' in L.lib.ococc_last_error()
    assert L.lib.ococc_track_extend_f64(None, None, None, None, None, 0, 0, None, None, None, 0, 0, None, None, None, 0, 0.9, 10,
                                        None, None, None, None) == 0
    rc = L.lib.ococc_tracklet_nonempty(None, 10, 6, None, None, 2, None, 1, 10, None, None)
    assert rc == -1 and b'null' in L.lib.ococc_last_error()
    rc = L.lib.ococc_tracklet_nonempty(None, 10, 2, None, None, 2, None, 1, 10, None, None)
    assert rc == -1 and b'3 columns' in L.lib.ococc_last_error()
    assert L.lib.ococc_tracklet_nonempty(None, 0, 6, None, None, 0, None, 0, 0, None, None) == 0


def test_packed_table_checks_run_before_any_launch(monkeypatch):
    """the host checks of extend_tracks_packed (which keep the kernel inside its buffers) on stand-in 'device' tensors"""
    monkeypatch.setattr(L, 'require_device', lambda *a: None)
    monkeypatch.setattr(L, 'stream', lambda: None)
    monkeypatch.setattr(L.lib, 'ococc_track_extend_f64', lambda *a: (_ for _ in ()).throw(AssertionError('launched')))
    z = torch.zeros
    ok = dict(boxes=z(3, 7), offsets=[0, 3], frames=[2, 3, 4], segments=[0], scores=z(3, dtype=torch.float64), poses=z(6, 16),
              timestamps=z(6, dtype=torch.int64), seg_offsets=[0, 6], num_back=[2], num_fwd=[1], out_offsets=[0, 6],
              score_multiplier=0.9, velo_window_size=10)
    for bad in (dict(num_back=[3], out_offsets=[0, 7]), dict(num_fwd=[2], out_offsets=[0, 7]), dict(out_offsets=[0, 5]),
                dict(frames=[2, 2, 4]), dict(frames=[2, 3, 6]), dict(segments=[1]), dict(seg_offsets=[0, 5]), dict(offsets=[0, 2]),
                dict(scores=z(3)), dict(poses=z(5, 16)), dict(num_back=[-1], out_offsets=[0, 3]), dict(velo_window_size=0)):
        with pytest.raises(L.OcoccError):
            cp.extend_tracks_packed(**{**ok, **bad})
    with pytest.raises(AssertionError, match='launched'):
        cp.extend_tracks_packed(**ok)


def test_new_exports_have_header_ctypes_and_integration_rows():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ococc_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(ococc_[a-z0-9_]+)\s*\(', header))
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_EXPORTS:
        assert name in declared and name in L.SIGNATURES and hasattr(L.lib, name)
        assert any(f'`{name}`' in line and line.startswith('|') for line in integration.splitlines()), f'{name}: no INTEGRATION.md row'
    assert len(L.SIGNATURES['ococc_track_extend_f64'][1]) == 22 and len(L.SIGNATURES['ococc_tracklet_nonempty'][1]) == 11


# ---------------------------------------------------------------------------------------------- the tools, on stand-ins
def _extend_stand_in(cfg):
    def fn(boxes, offsets, frames, segments, scores, poses, timestamps, seg_offsets, num_back, num_fwd, out_offsets,
           score_multiplier, velo_window_size):
        fx = dict(boxes=boxes.numpy(), offsets=np.asarray(offsets), frames=np.asarray(frames), segments=np.asarray(segments),
                  scores=scores.numpy(), poses=poses.numpy(), timestamps=timestamps.numpy(), seg_offsets=np.asarray(seg_offsets))
        out = extend_f64(fx, dict(extend_length=cfg['extend_length'], min_length=cfg['min_length_to_extend'], extend_all=False,
                                  min_length_all=0, velo_window_size=velo_window_size, score_multiplier=score_multiplier))
        assert [len(o[0]) for o in out] == np.diff(out_offsets).tolist()           # the host plan and the restatement's agree
        return (torch.from_numpy(np.concatenate([o[0] for o in out], 0).astype(np.float32)),
                torch.from_numpy(np.concatenate([o[1] for o in out])), torch.from_numpy(np.concatenate([o[2] for o in out]).astype(np.int32)))
    return fn


def _nonempty_stand_in(points, point_offsets, boxes, box_offsets):
    from test_ctrl_prep_cpu import crop_packed_f64
    counts, _ = crop_packed_f64(points, point_offsets, boxes, box_offsets)
    return (counts > 0).to(torch.int32)


def test_tools_on_the_synthetic_tree_with_stand_ins(tmp_path, monkeypatch):
    """raw tree -> extend_tracks -> remove_empty with the two device operators replaced by float64 restatements: file
    names, object order, the written records, and -- for the committed seed of the synthetic tree -- that fewer than
    2 % of the boxes hang on points within 1e-3 m of a face (the exception the GPU end-to-end test allows)."""
    import yaml
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_synthetic_raw
    from test_gpu_remove_empty import in_box_f64, lifted_f64, undecided
    raw = str(tmp_path / 'raw')
    make_synthetic_raw.main([raw])
    config = os.path.join(raw, 'synthetic_extend.yaml')
    cfg = yaml.safe_load(open(config))
    monkeypatch.setattr(cp, 'extend_tracks_packed', _extend_stand_in(cfg))
    monkeypatch.setattr(cp, 'nonempty_frames_packed', _nonempty_stand_in)
    monkeypatch.setattr(cp, 'CROP_BATCH_BYTES', 400_000)           # several batches
    extended = cp.extend_tracks(config, device='cpu')
    assert extended == os.path.join(raw, 'waymo_format', 'pred_synthetic_extend.bin')
    before, after = waymo_io.read_bin(os.path.join(raw, 'waymo_format', 'pred.bin')), waymo_io.read_bin(extended)
    assert len(after) > len(before)
    # the reference's order: tracklets in order of first appearance, frames ascending; extras carry the decayed score
    tracks = list(dict.fromkeys((o['context_name'], o['id']) for o in before))
    assert list(dict.fromkeys((o['context_name'], o['id']) for o in after)) == tracks
    for trk in tracks:
        old = [o for o in before if (o['context_name'], o['id']) == trk]
        new = [o for o in after if (o['context_name'], o['id']) == trk]
        stamps = [o['frame_timestamp_micros'] for o in new]
        assert stamps == sorted(stamps) and len(set(stamps)) == len(stamps)
        extra = len(new) - len(old)
        assert [o['frame_timestamp_micros'] for o in new[extra:]] == [o['frame_timestamp_micros'] for o in old]
        assert [o['score'] for o in new[extra:]] == [o['score'] for o in old] and all(o['type'] == 1 for o in new)
        for i in range(extra):
            assert new[i]['score'] == float(np.float32(old[0]['score'] * cfg['score_multiplier'] ** (i + 1)))
            assert (new[i]['width'], new[i]['length'], new[i]['height']) == (old[0]['width'], old[0]['length'], old[0]['height'])
        for o, p in zip(new[extra:], old):
            assert abs(o['center_x'] - p['center_x']) < 1e-4 and abs(o['center_z'] - p['center_z']) < 1e-4
            assert abs(o['heading'] - p['heading']) < 1e-4
    assert any(len([o for o in after if (o['context_name'], o['id']) == t]) > len([o for o in before if (o['context_name'], o['id']) == t])
               for t in tracks)
    filtered = cp.remove_empty(extended, 'training', mm_data_root=os.path.join(raw, 'kitti_format'), device='cpu')
    assert filtered == os.path.join(raw, 'waymo_format', 'pred_synthetic_extend_wo_empty_right.bin')
    kept = waymo_io.read_bin(filtered)
    idx = [next(i for i, o in enumerate(after) if o == k) for k in kept]
    assert 0 < len(kept) < len(after) and len(set(idx)) == len(idx)
    frames = list(dict.fromkeys(o['frame_timestamp_micros'] for o in after))
    expect_order = [i for ts in frames for i, o in enumerate(after) if o['frame_timestamp_micros'] == ts and i in set(idx)]
    assert idx == expect_order                                      # frames in file order, boxes in file order
    ts2idx, _ = cp.load_frame_index(os.path.join(raw, 'kitti_format'))
    unsure, kept_set = 0, set(idx)
    for i, o in enumerate(after):
        cloud = np.fromfile(os.path.join(raw, 'kitti_format', 'training', 'velodyne', ts2idx[o['frame_timestamp_micros']] + '.bin'),
                            np.float32).reshape(-1, 6)[:, :3]
        box = lifted_f64(o, 0.2)
        if undecided(cloud, box):
            unsure += 1
        else:
            assert bool(in_box_f64(cloud, box).any()) == (i in kept_set)
    assert unsure <= 0.02 * len(after), f'{unsure} of {len(after)} boxes are undecided within the 1e-3 m shell'
    assert not any(o['id'].endswith('_fp') for o in kept)
