"""The occupancy-enhanced clouds of a chunked online call on the MI355X (TrackletRoIHeadOCC.simple_test_scene_steps_merged,
occ_ops.occ_merge_frames, tools/online_raw.py --chunk T --save-merged DIR --merged-per-call) on the small model and the
tracklets of tests/test_gpu_scene_rows.py.  The call: three clouds, rows slot-major, the first cloud without a row, the
second tracklet starting in the second cloud.

As in tests/test_gpu_online_merged.py the outputs of the point encoders (float atomics: two passes agree to rounding only,
DESIGN 3.14) are computed once per call and replayed, so states stepped through different methods see the same encoder
outputs and everything behind them is compared between states."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_merge_frames_ref as ref                                            # noqa: E402
from test_gpu_online_merged import _distance, _np, _row_scores, _sorted_rows  # noqa: E402
from test_gpu_scene_rows import FRAMES, head_frames                           # noqa: E402
from test_gpu_scene_steps import KEYS, OCC_KEYS, call_inputs                  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MERGED_KEYS = {'points_merged', 'merged_offsets', 'merged_counts'}
SAME = ('boxes', 'scores', 'labels', 'valid', 'fused_roi_feats', 'ori_roi_feats', 'boxes_ego', 'num_points', 'occ_ego',
        'occ_flags', 'occ_counts')


@pytest.fixture(scope='module', autouse=True)
def _generators_as_found():
    """later tests of the suite initialise networks from torch's global generators without seeding them"""
    cpu = torch.get_rng_state()
    gpu = torch.cuda.get_rng_state() if torch.cuda.is_available() else None
    yield
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state(gpu)


@pytest.fixture(scope='module')
def model(dev):
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (register)
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    torch.manual_seed(0)
    return DETECTORS.build(ococcnet_model_cfg()).to(dev).eval()


def chunk_inputs(dev):
    """sensor frames 0, 1, 2 in one call without the rows of cloud 0: tracklet 0 (slot 2) in clouds 1 and 2, tracklet 1
    (slot 0) likewise -- it starts in the second cloud --, slot-major, so the frame-major order is a real permutation"""
    kw, _, _ = call_inputs(dev, head_frames(), (0, 1, 2), {})
    keep = [i for i, f in enumerate(kw['frame_rows']) if f != 0]
    for k in ('boxes', 'scores', 'labels'):
        kw[k] = kw[k][keep]
    kw['frame_rows'], kw['slot_rows'] = [kw['frame_rows'][i] for i in keep], [kw['slot_rows'][i] for i in keep]
    assert kw['frame_rows'] == [1, 2, 1, 2] and kw['slot_rows'] == [2, 2, 0, 0] and len(kw['cloud_sizes']) == 3
    return kw


@pytest.fixture(scope='module')
def walk(dev, model):
    """the call on five fresh states: the new method with merged=True, simple_test_scene_steps(occ=True) twice (the second is
    the yardstick of what two states of the parent's call differ by), the new method with drop_observed and another
    use_dim, and with a threshold between two of the call's row scores (taken from the first run)"""
    rh = model.roi_head
    head, store = rh.bbox_head, {}
    real = head._encode_rois

    def replayed(*a):
        if 'call' not in store:
            store['call'] = real(*a)
        return store['call']

    head._encode_rois = replayed
    try:
        kw = chunk_inputs(dev)
        st = types.SimpleNamespace(**{k: rh.online_begin(3, dev, cap=FRAMES) for k in ('merged', 'occ', 'occ2', 'drop', 'thr')})
        rec = types.SimpleNamespace(kw=kw, st=st, cloud=kw['points'].cpu().numpy())
        rec.merged = rh.simple_test_scene_steps_merged(**kw, state=st.merged)
        rec.occ = rh.simple_test_scene_steps(**kw, state=st.occ, occ=True)
        rec.occ2 = rh.simple_test_scene_steps(**kw, state=st.occ2, occ=True)
        rec.drop = rh.simple_test_scene_steps_merged(**kw, state=st.drop, merged=dict(drop_observed=True, use_dim=[0, 1, 2, 4]))
        rs = np.unique(_row_scores(rec.merged, kw['scores']))
        gap = int(np.argmax(np.diff(rs)))                      # the widest gap between two row scores of the first run
        rec.thr_value = float(np.float32(0.5) * (rs[gap] + rs[gap + 1]))
        rec.thr = rh.simple_test_scene_steps_merged(**kw, state=st.thr, merged=dict(score_threshold=rec.thr_value))
        return rec
    finally:
        del head._encode_rois


def _check(rec, out, use_dim, threshold, drop):
    """points_merged, merged_offsets and merged_counts of a call against the restatement on the SAME call's occ_ego,
    occ_counts, occ_flags and row scores"""
    kw = rec.kw
    rs = _row_scores(out, kw['scores'])
    want, offsets, kept = ref.occ_merge_frames_ref(
        rec.cloud, kw['cloud_sizes'], out['occ_ego'].cpu().numpy(), out['occ_counts'], kw['frame_rows'], use_dim, row_score=rs,
        flags=out['occ_flags'].cpu().numpy(), drop_observed=drop, score_threshold=threshold)
    got = out['points_merged'].cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape == (len(rec.cloud) + sum(kept), len(use_dim) + 2)
    assert got.tobytes() == want.tobytes()
    assert isinstance(out['merged_offsets'], list) and out['merged_offsets'] == offsets and len(offsets) == 4
    assert isinstance(out['merged_counts'], list) and out['merged_counts'] == kept and len(kept) == len(kw['frame_rows'])
    assert offsets[1] == kw['cloud_sizes'][0]                      # the cloud without a row: its points only
    return rs, kept


def test_points_merged_of_the_call(walk):
    assert set(walk.merged) == KEYS | OCC_KEYS | MERGED_KEYS
    rs, kept = _check(walk, walk.merged, [0, 1, 2, 3, 4], 0.0, False)
    assert kept == [c if s > 0 else 0 for c, s in zip(walk.merged['occ_counts'], rs)] and sum(kept) > 100
    assert walk.st.merged.frames == [2, 0, 2]


def test_drop_observed_and_another_use_dim(walk):
    out = walk.drop
    rs, kept = _check(walk, out, [0, 1, 2, 4], 0.0, True)
    flags = out['occ_flags'].cpu().numpy()
    cuts = np.cumsum([0] + list(out['occ_counts']))
    seen = [int(((flags[cuts[r]:cuts[r + 1]] & 2) != 0).sum()) for r in range(len(kept))]
    assert kept == [(c - s) if sc > 0 else 0 for c, s, sc in zip(out['occ_counts'], seen, rs)] and sum(seen) > 100


def test_threshold_between_two_row_scores(walk):
    first = _row_scores(walk.merged, walk.kw['scores'])
    assert (first > np.float32(walk.thr_value)).any() and not (first > np.float32(walk.thr_value)).all()
    rs, kept = _check(walk, walk.thr, [0, 1, 2, 3, 4], walk.thr_value, False)
    above = rs > np.float32(walk.thr_value)
    assert [k > 0 for k in kept] == [bool(a) and n > 0 for a, n in zip(above, walk.thr['occ_counts'])]
    if 0 < above.sum() < len(above):                # (the scores of this run fall on both sides, as those of the first did)
        assert 0 < sum(kept) < sum(walk.thr['occ_counts'])


def test_call_does_not_notice_merged(walk):
    """a state stepped through the new method and one through simple_test_scene_steps(occ=True): every other key and the
    cache no further apart than two occ=True states are from each other (the parent's code path is the yardstick)"""
    worst, noise = {}, {}
    for k in SAME:
        worst[k], noise[k] = _distance(walk.merged[k], walk.occ[k]), _distance(walk.occ2[k], walk.occ[k])
    for name in ('k', 'v'):
        pairs = lambda a, b: max(_distance(x, y) for x, y in zip(getattr(a.cache, name), getattr(b.cache, name)))
        worst['cache.' + name], noise['cache.' + name] = pairs(walk.st.merged, walk.st.occ), pairs(walk.st.occ2, walk.st.occ)
    print('steps_merged against steps(occ=True), largest relative distance: ' + ', '.join(f'{k} {v:.3e}' for k, v in worst.items()))
    print('steps(occ=True) against steps(occ=True), two states:             ' + ', '.join(f'{k} {v:.3e}' for k, v in noise.items()))
    for k in worst:
        assert worst[k] <= noise[k], (k, worst[k], noise[k])
    assert walk.st.merged.frames == walk.st.occ.frames and torch.equal(walk.st.merged.cache.pos, walk.st.occ.cache.pos)
    for a, b in zip(walk.st.merged.origin, walk.st.occ.origin):
        assert (a is None and b is None) or np.array_equal(a, b)


def test_empty_call_is_the_clouds_with_two_zero_columns(dev, model):
    rh = model.roi_head
    state = rh.online_begin(3, dev, cap=FRAMES)
    frames = head_frames()
    clouds = [frames[0][0], frames[1][0]]
    points = torch.from_numpy(np.concatenate(clouds)).to(dev)
    before = [k.clone() for k in state.cache.k]
    out = rh.simple_test_scene_steps_merged(points, [len(c) for c in clouds], np.stack([frames[0][1], frames[1][1]]),
                                            torch.zeros((0, 7), device=dev), torch.zeros((0,), device=dev),
                                            torch.zeros((0,), dtype=torch.long, device=dev), [], [], state)
    got = out['points_merged'].cpu().numpy()
    assert set(out) == KEYS | OCC_KEYS | MERGED_KEYS
    assert got.shape == (len(points), 7) and got[:, :5].tobytes() == np.concatenate(clouds).tobytes() and (got[:, 5:] == 0).all()
    assert out['merged_offsets'] == [0, len(clouds[0]), len(points)] and out['merged_counts'] == [] and out['occ_counts'] == []
    assert state.frames == [0, 0, 0] and state.origin == [None] * 3
    assert all(torch.equal(a, b) for a, b in zip(before, state.cache.k))


def test_replay_in_chunks_writes_the_offline_loaders_files(dev, model, tmp_path):
    """make_synthetic_raw's tree replayed with chunk = 3, --save-occ, --save-merged and --merged-per-call: one file per
    timestamp, each the rows LoadPointsAndOccPredFromFile builds from the cloud file and that run's own --save-occ files
    (compared as tests/test_gpu_online_merged.py compares); merged_cells of the records sum to the cells in the files.
    Against a chunk = 1 replay only the real rows and the file count are compared: the chunked call's probabilities
    differ from the single steps' in some runs, so a cell at the decoder's threshold may differ."""
    import importlib.util
    from objectcentricocccompletion_amd import ctrl_prep, occ_export, pipelines
    tools = os.path.join(ROOT, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import make_synthetic_raw
    spec = importlib.util.spec_from_file_location('ococc_tools_online_raw', os.path.join(tools, 'online_raw.py'))
    online_raw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(online_raw)
    root = str(tmp_path / 'raw')
    make_synthetic_raw.main([root, '--segments', '1', '--tracklets', '2', '--frames', '6', '--background', '500'])
    yaml, poses = os.path.join(root, 'synthetic_vehicle.yaml'), os.path.join(root, 'poses.pkl')
    occ_dir, merged_dir, single_dir = str(tmp_path / 'occ'), str(tmp_path / 'merged'), str(tmp_path / 'merged1')
    with pytest.raises(ValueError, match='chunk'):
        online_raw.replay(model, yaml, slots=4, poses=poses, chunk=3, save_merged=merged_dir)
    records, state = online_raw.replay(model, yaml, slots=4, poses=poses, chunk=3, save_occ=occ_dir, save_merged=merged_dir,
                                       merged_per_call=True)
    assert state.frames == [0, 0, 0, 0] and all('merged_cells' in r and 'occ_cells' in r for r in records)
    online_raw.replay(model, yaml, slots=4, poses=poses, save_merged=single_dir)
    cfg, _ = ctrl_prep.load_config(yaml)
    ts2idx, _ = ctrl_prep.load_frame_index(cfg.get('mm_data_root', ctrl_prep.MM_DATA_ROOT))
    pc_root = ctrl_prep.velodyne_dir(cfg)
    load = pipelines.LoadPointsAndOccPredFromFile('LIDAR', points_load_dim=6, points_use_dim=5, occs_use_dim=4)
    frames = sorted({(r['segment'], r['timestamp']) for r in records})
    assert len(frames) == 6
    cells = 0
    for seg, ts in frames:
        got = np.fromfile(os.path.join(merged_dir, str(seg), f'{ts}.bin'), dtype=np.float32).reshape(-1, 7)
        want = load(dict(pts_filename=os.path.join(pc_root, f'{ts2idx[ts]}.bin'),
                         occ_pred_filename=occ_export.occ_pred_filename(occ_dir, seg, ts, True)))['points']
        assert got.shape == want.shape, (seg, ts, got.shape, want.shape)
        assert np.array_equal(_sorted_rows(got), _sorted_rows(want)), (seg, ts)
        n_cells = int((got[:, 6] == 1).sum())
        assert n_cells == sum(r['merged_cells'] for r in records if (r['segment'], r['timestamp']) == (seg, ts))
        cells += n_cells
        single = np.fromfile(os.path.join(single_dir, str(seg), f'{ts}.bin'), dtype=np.float32).reshape(-1, 7)
        real = single[:, 6] == 0
        assert got[:real.sum()].tobytes() == single[real].tobytes() and (got[real.sum():, 6] == 1).all()
    listing = lambda d: sorted(os.path.relpath(os.path.join(p, n), d) for p, _, names in os.walk(d) for n in names)
    assert listing(merged_dir) == sorted(os.path.join(str(seg), f'{ts}.bin') for seg, ts in frames) == listing(single_dir)
    assert cells > 100
