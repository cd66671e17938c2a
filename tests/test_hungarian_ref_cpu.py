"""CPU suite of the Hungarian matcher of the native Waymo metric (DESIGN.md 3.10 rule 4b): the plain restatement
tests/hungarian_ref.py is pinned to scipy.optimize.linear_sum_assignment -- for every prefix of every generated group
the total weight equals scipy's optimum exactly (integers), the matching is one-to-one and uses edges only -- and to
the two hand examples; the snapshot layout and the argument checks of the new export."""
import os
import sys

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hungarian_ref as H        # noqa: E402
import waymo_metrics_ref as R    # noqa: E402


def _check_prefixes(weights, n_cols):
    """every prefix: optimal (scipy, weights padded with one zero column per prediction), one-to-one, edges only;
    -> the number of prefixes in which a prediction changed its partner"""
    W = np.asarray(weights, dtype=np.int64).reshape(len(weights), n_cols)
    changes, before = 0, []
    for n, m in enumerate(H.prefix_matchings(weights, n_cols), 1):
        assert len(m) == n
        cols = [j for j in m if j >= 0]
        assert len(cols) == len(set(cols)) and all(0 <= j < n_cols for j in cols)
        assert all(W[i, j] > 0 for i, j in enumerate(m) if j >= 0)
        padded = np.concatenate([W[:n], np.zeros((n, n), dtype=np.int64)], axis=1)
        r, c = linear_sum_assignment(padded, maximize=True)
        assert H.total_weight(weights, m) == int(padded[r, c].sum()), f'prefix {n}'
        changes += any(a != b for a, b in zip(before, m))
        before = m
    return changes


def test_generated_groups_every_prefix_is_optimal():
    groups = H.generated_groups()
    sizes = {(len(p), len(g)) for _, p, g, _, _ in groups}
    assert (0, 5) in sizes and (6, 0) in sizes and (1, 1) in sizes and (200, 150) in sizes
    moved = 0
    for name, pds, gts, thr, scores in groups:
        ious = np.array([[R.iou3d(p, g) for g in gts] for p in pds], dtype=np.float32).reshape(len(pds), len(gts))
        weights = H.weights_from_ious(ious, thr)
        changes = _check_prefixes(weights, len(gts))
        W = np.asarray(weights).reshape(len(pds), len(gts))
        edges, distinct = int((W > 0).sum()), len(set(W[W > 0].tolist()))
        print(f'{name}: {edges} edges, {distinct} distinct weights, {changes} prefixes moved a partner')
        if name.startswith('lattice') and len(pds) >= 20:
            assert edges > 3 * len(pds) and distinct <= 40, 'the case is neither dense nor full of ties'
        if name.startswith('dense') and len(pds) >= 30:
            assert edges > 3 * len(pds)
        if name.startswith('sparse') and len(pds) >= 80:
            assert 0 < edges < len(pds)
        moved += changes
        assert scores == sorted(scores, reverse=True) and len(scores) == len(pds)
    assert moved > 100          # the insertions do re-route earlier predictions


@pytest.mark.parametrize('seed', range(6))
def test_random_weight_matrices_every_prefix_is_optimal(seed):
    """weights given directly: dense with few distinct values (ties everywhere), sparse, and full-range"""
    rng = np.random.default_rng(seed)
    n, m = int(rng.integers(1, 60)), int(rng.integers(1, 50))
    values = [np.array([0, 500, 700, 900]), np.array([0, 0, 0, 0, 0, 0, 0, 800, 801]), np.arange(0, 1001)][seed % 3]
    weights = rng.choice(values, (n, m)).tolist()
    _check_prefixes(weights, m)


def test_hand_example_a_partner_changes_with_the_cutoff():
    """A (0.9): g1 800, g2 750; B (0.8): g1 720.  Alone, A takes g1; with B, A moves to g2 (750 + 720 > 800)."""
    after = list(H.prefix_matchings(H.HAND_1['weights']))
    assert after == [[0], [1, 0]]
    per_cutoff = H.cutoff_matchings(**H.HAND_1)
    assert per_cutoff[100] == [] and per_cutoff[91] == [] and per_cutoff[90] == [0] and per_cutoff[81] == [0]
    assert per_cutoff[80] == [1, 0] and per_cutoff[0] == [1, 0]


def test_hand_example_the_better_duplicate_takes_the_box():
    """one box, A (0.9) at 720, B (0.8) at 900: A holds it until B arrives"""
    assert list(H.prefix_matchings(H.HAND_2['weights'])) == [[0], [-1, 0]]
    per_cutoff = H.cutoff_matchings(**H.HAND_2)
    assert per_cutoff[85] == [0] and per_cutoff[80] == [-1, 0]


def test_ties_lower_index_and_real_before_private():
    assert list(H.prefix_matchings([[700, 700, 700]])) == [[0]]
    assert list(H.prefix_matchings([[700, 700], [700, 700]])) == [[0], [0, 1]]     # the second takes the free column
    # equal totals either way (700 + 0 = 0 + 700): the new row's own private column and the first row's (reached through
    # column 0) are both at distance 0; the row scanned first wins, so nothing moves
    assert list(H.prefix_matchings([[700], [700]])) == [[0], [0, -1]]
    assert list(H.prefix_matchings([[700], [701]])) == [[0], [-1, 0]]
    assert H.weight(0.7, 0.7) == 700 and H.weight(np.float32(0.69999), 0.7) == 0 and H.weight(1.0, 0.5) == 1000
    assert H.weight(0.0009, 0.0001) == 0                # a weight of 0 is no edge


def test_snapshot_layout():
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd import waymo_metrics as M
    scores = [0.95, 0.95, 0.5, 0.2, 0.9, -1.0, 0.3]
    buckets = M.cutoff_buckets(scores)
    assert buckets.tolist() == [96, 96, 51, 21, 91, 0, 31]
    # frame 0: types 1, 1, 1, 2; frame 1: types 1, 1; frame 2: type 5
    lay = M.snapshot_layout([0, 4, 6, 7], [1, 1, 1, 2, 1, 1, 5], buckets)
    assert lay['group_start'].tolist() == [0, 0, 0, 3, 4, 4, 6]
    assert lay['snap_off'].tolist() == [-1, 0, 2, 5, 6, -1, -1] and lay['total'] == 7
    assert lay['ends'].tolist() == [1, 2, 3, 4]
    assert lay['k_lo'].tolist() == [51, 0, 0, 0] and lay['k_hi'].tolist() == [95, 50, 20, 90]
    with pytest.raises(L.OcoccError):
        M.snapshot_layout([0, 2], [1, 1], [10, 20])     # buckets must not increase inside a group
    empty = M.snapshot_layout([0], [], [])
    assert empty['total'] == 0 and len(empty['snap_off']) == 0


def test_frame_assign_abi_argument_errors():
    """the export's checks run before anything touches a device"""
    from objectcentricocccompletion_amd import _lib as L
    thr = (L.c_f32 * 5)(0, .7, .5, .5, .5)
    call = lambda max_gt, max_pd, thr, ws, frame_end=0, pair_end=100, words=0: L.lib.ococc_frame_assign_i32(
        None, None, None, None, 0, None, None, None, None, 0, None, 0, frame_end, 0, pair_end, max_gt, max_pd, thr, None,
        words, None, None, ws, None)
    assert call(5000, 10, thr, 1 << 20) == -1 and b'4096' in L.lib.ococc_last_error()
    assert call(4096, 10, thr, 1 << 20) == -1 and b'64 KiB' in L.lib.ococc_last_error()
    assert call(64, 40000, thr, 1 << 20) == -1 and b'64 KiB' in L.lib.ococc_last_error()
    assert call(10, 10, (L.c_f32 * 5)(0, 0, .5, .5, .5), 1 << 20) == -1 and b'thresholds' in L.lib.ococc_last_error()
    assert call(10, 10, thr, 16) == -1 and b'workspace' in L.lib.ococc_last_error()
    assert call(10, 10, thr, 1 << 20, frame_end=-1) == -1 and b'frame range' in L.lib.ococc_last_error()
    assert call(10, 10, thr, 1 << 20, pair_end=-1) == -1 and b'pair range' in L.lib.ococc_last_error()
    assert call(10, -1, thr, 1 << 20) == -1 and call(10, 10, thr, 1 << 20, words=-1) == -1
    assert call(10, 10, thr, 1 << 20) == 0          # no frames: nothing to launch


def test_unknown_matcher_raises():
    from objectcentricocccompletion_amd import waymo_metrics as M
    with pytest.raises(ValueError, match='greedy'):
        M.detection_metrics([], [], matcher='greedy')
    with pytest.raises(ValueError):
        M.evaluate_files('a.bin', 'b.bin', matcher='Hungarian')
    assert M.MATCHERS == ('score_first', 'hungarian')


def test_the_dataset_and_the_tools_pass_the_matcher_on(tmp_path, monkeypatch):
    import torch
    from objectcentricocccompletion_amd import waymo_io as W
    from objectcentricocccompletion_amd import waymo_metrics as M
    from objectcentricocccompletion_amd.dataset import WaymoTrackletDatasetWithOcc
    from objectcentricocccompletion_amd.tracklet import Tracklet
    seen = []
    monkeypatch.setattr(M, 'evaluate_files', lambda pred, gt, assume_points=False, txt_path=None, matcher='score_first':
                        seen.append(matcher) or {})
    ds = WaymoTrackletDatasetWithOcc.__new__(WaymoTrackletDatasetWithOcc)
    ds.CLASSES = ('Car',)
    ds.data_root = str(tmp_path / 'kitti_format') + '/'
    trk = Tracklet(torch.ones(2, 7), [10, 11], segment_name='segment-000', id='a')
    results = [dict(out_tracklets=[trk])]
    ds.evaluate(results, metric='waymo_native', pklfile_prefix=str(tmp_path / 'a'))
    ds.evaluate(results, metric='waymo_native', pklfile_prefix=str(tmp_path / 'b'), matcher='hungarian')
    assert seen == ['score_first', 'hungarian']
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
    sys.path.insert(0, tools)
    try:
        import waymo_detection_metrics as tool
        tool.main(['p.bin', 'g.bin', '--matcher', 'hungarian'])
        tool.main(['p.bin', 'g.bin'])
        with pytest.raises(SystemExit):
            tool.main(['p.bin', 'g.bin', '--matcher', 'greedy'])
    finally:
        sys.path.remove(tools)
    assert seen[2:] == ['hungarian', 'score_first']


def test_curves_per_cutoff_equal_the_restated_table():
    """the host half of matcher='hungarian' without a device: snapshots filled from the restatement (float64 IoUs rounded
    to float32 stand in for the kernel's) through waymo_metrics.curves against the straight loops over cutoffs"""
    import test_gpu_waymo_hungarian as T
    from objectcentricocccompletion_amd import waymo_metrics as M
    preds, gts = T._scene_with_duplicates(np.random.default_rng(5))
    pk = M.pack(M.columns(preds), M.columns(gts))
    ious = {}
    for f in range(pk['F']):
        for p in range(pk['pd_offsets'][f], pk['pd_offsets'][f + 1]):
            for g in range(pk['gt_offsets'][f], pk['gt_offsets'][f + 1]):
                if pk['pd_eligible'][p] and pk['gt_eligible'][g] and pk['pd_type'][p] == pk['gt_type'][g]:
                    v = np.float32(R.iou3d(list(pk['pd_boxes'][p]), list(pk['gt_boxes'][g])))
                    if v > 0:
                        ious[(p, g)] = v
    layout = M.snapshot_layout(pk['pd_offsets'], pk['pd_type'], M.cutoff_buckets(pk['pd_score']))
    snaps = np.full(layout['total'], -7, dtype=np.int32)
    matches = [[-1] * len(preds) for _ in range(101)]
    for rows, g0, per_cutoff in T._expected_per_cutoff(pk, ious, T.SHIPPED):
        for k in range(101):
            m = per_cutoff[k] if per_cutoff else []
            if not m:
                continue
            off = int(layout['snap_off'][rows[len(m) - 1]])
            assert off >= 0
            snaps[off:off + len(m)] = [g0 + c if c >= 0 else -1 for c in m]
            for r, c in enumerate(m):
                if c >= 0:
                    matches[k][int(pk['pd_order'][rows[r]])] = int(pk['gt_order'][g0 + c])
    assert (snaps != -7).all()
    exp = T._table_per_cutoff(preds, gts, matches)
    got = M.curves(pk, per_cutoff=(snaps, layout))
    assert list(got) == list(exp)
    worst = max(max(abs(got[k][0] - exp[k][0]), abs(got[k][1] - exp[k][1])) for k in exp)
    print(f'largest |table difference| {worst:.3e}')
    assert worst <= 1e-12
    first = R.detection_metrics(preds, gts)[0]
    assert sum(abs(first[k][1] - exp[k][1]) > 1e-6 for k in exp) >= 8     # the matchers disagree on this scene


def test_curves_per_cutoff_do_not_depend_on_the_block_size():
    """the per-cutoff curves go over the snapshots in blocks; the counts are exact and the blocks only regroup the
    float64 heading sums"""
    from objectcentricocccompletion_amd import waymo_metrics as M
    rng = np.random.default_rng(2)
    preds, gts = [], []
    for f in range(12):
        p, g = R.random_frame(rng, 25, 15, ts=f)
        preds, gts = preds + p, gts + g
    pk = M.pack(M.columns(preds), M.columns(gts))
    layout = M.snapshot_layout(pk['pd_offsets'], pk['pd_type'], M.cutoff_buckets(pk['pd_score']))
    snaps = np.full(layout['total'], -1, dtype=np.int32)
    for end in layout['ends']:                 # any one-to-one partner choice will do: the first boxes of the frame
        gs, off = int(layout['group_start'][end]), int(layout['snap_off'][end])
        f = int(np.searchsorted(pk['pd_offsets'], end, side='right')) - 1
        g0, g1 = int(pk['gt_offsets'][f]), int(pk['gt_offsets'][f + 1])
        for r in range(0, end - gs + 1, 2):
            if g0 + r < g1 and pk['gt_eligible'][g0 + r] and pk['gt_type'][g0 + r] == pk['pd_type'][gs + r]:
                snaps[off + r] = g0 + r
    assert (snaps >= 0).sum() > 50
    whole = M._curves_per_cutoff(pk, snaps, layout)
    for words in (1, 37, 1000):
        part = M._curves_per_cutoff(pk, snaps, layout, block_words=words)
        assert list(part) == list(whole)
        assert max(max(abs(part[k][0] - whole[k][0]), abs(part[k][1] - whole[k][1])) for k in whole) <= 1e-12
    assert max(v[0] for v in whole.values()) > 0


def test_hungarian_rejects_nan_scores_by_name(monkeypatch):
    import torch
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd import waymo_metrics as M
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(L, 'require_device', lambda *a: None)
    box = [1.0, 2.0, 0.5, 4.0, 2.0, 1.5, 0.0]
    preds = [R.make_object(box, 1, 0.5), R.make_object(box, 1, float('nan'))]
    with pytest.raises(L.OcoccError, match='NaN score'):
        M.detection_metrics(preds, [R.make_object(box, 1)], matcher='hungarian', device='cpu')
