"""GPU suite: the Hungarian matcher of the native Waymo detection metric (frame_assign_kernel in csrc/frame_match.hip,
waymo_metrics.frame_assign, matcher='hungarian'; DESIGN.md 3.10 rule 4b) against the plain restatement
tests/hungarian_ref.py.  The arithmetic is integer: every snapshot must equal the restatement exactly.  The float32 IoUs
that feed the restatement are the overlap kernel's own values read back (every pair once more as a frame of its own
through frame_match, whose match_iou is the matrix entry), so nothing depends on how a CPU IoU rounds near a threshold.
The table is compared to 1e-12 absolute, the tolerance tests/test_gpu_waymo_metrics.py holds its table to: the two sides
differ by float64 summation order only."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hungarian_ref as H        # noqa: E402
import waymo_metrics_ref as R    # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIPPED = (0.0, 0.7, 0.5, 0.5, 0.5)


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _device_args(pk):
    dev = _dev()
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(dev)
    return (up(pk['pd_boxes'], np.float32), up(pk['pd_type'], np.int32), up(pk['pd_eligible'], np.int32), pk['pd_offsets'],
            up(pk['gt_boxes'], np.float32), up(pk['gt_type'], np.int32), up(pk['gt_eligible'], np.int32), pk['gt_offsets'])


def _assign(preds, gts, thresholds=SHIPPED, **kw):
    """-> packed arrays, snapshots (device tensor), layout"""
    from objectcentricocccompletion_amd import waymo_metrics as M
    pk = M.pack(M.columns(preds), M.columns(gts))
    snaps, layout = M.frame_assign(*_device_args(pk), M.cutoff_buckets(pk['pd_score']), iou_thresholds=thresholds, **kw)
    return pk, snaps, layout


def _kernel_ious(pk):
    """{(packed prediction, packed ground truth): float32 IoU} for every eligible equal-type pair of a frame, as the
    overlap kernel computes it: each pair once more as a 1 x 1 frame of type 1 at the lowest threshold the export takes"""
    from objectcentricocccompletion_amd import waymo_metrics as M
    dev = _dev()
    pi, gi = [], []
    for f in range(pk['F']):
        p = np.arange(pk['pd_offsets'][f], pk['pd_offsets'][f + 1])
        g = np.arange(pk['gt_offsets'][f], pk['gt_offsets'][f + 1])
        p, g = p[pk['pd_eligible'][p] != 0], g[pk['gt_eligible'][g] != 0]
        for t in (1, 2, 3, 4):
            pt, gt = p[pk['pd_type'][p] == t], g[pk['gt_type'][g] == t]
            pi.append(np.repeat(pt, len(gt)))
            gi.append(np.tile(gt, len(pt)))
    pi, gi = np.concatenate(pi).astype(np.int64), np.concatenate(gi).astype(np.int64)
    n = len(pi)
    if n == 0:
        return {}
    ones = torch.ones(n, dtype=torch.int32, device=dev)
    off = np.arange(n + 1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).to(dev)
    _, mi = M.frame_match(up(pk['pd_boxes'][pi]), ones, ones, off, up(pk['gt_boxes'][gi]), ones, ones, off,
                          iou_thresholds=(0, 1e-30, .5, .5, .5))
    mi = mi.cpu().numpy()
    return {(int(a), int(b)): v for a, b, v in zip(pi, gi, mi) if v > 0}


def _groups(pk):
    """the (frame, type) groups of the packed predictions: (frame, type, packed prediction indices)"""
    out = []
    for f in range(pk['F']):
        a, b = int(pk['pd_offsets'][f]), int(pk['pd_offsets'][f + 1])
        start = a
        for p in range(a, b + 1):
            if p == b or pk['pd_type'][p] != pk['pd_type'][start]:
                if p > start:
                    out.append((f, int(pk['pd_type'][start]), list(range(start, p))))
                start = p
    return out


def _expected_per_cutoff(pk, ious, thresholds):
    """-> per group (rows, g0, [matching of cutoff k for k = 0 .. 100]) from the restatement; columns are all ground-truth
    boxes of the frame (no edge where the type differs or a box is ineligible)"""
    out = []
    for f, t, rows in _groups(pk):
        g0, g1 = int(pk['gt_offsets'][f]), int(pk['gt_offsets'][f + 1])
        if not 1 <= t <= 4:
            out.append((rows, g0, None))
            continue
        weights = [[H.weight(ious.get((p, g), 0.0), thresholds[t]) for g in range(g0, g1)] for p in rows]
        out.append((rows, g0, H.cutoff_matchings(weights, [float(pk['pd_score'][p]) for p in rows], g1 - g0)))
    return out


def _compare_snapshots(pk, snaps, layout, expected):
    """every cutoff of every group: the snapshot the layout names for it equals the restatement's matching; every snapshot
    is visited.  -> (snapshots compared, cutoffs at which a prediction's partner differs from the cutoff above)"""
    snaps = snaps.cpu().numpy()
    assert len(snaps) == layout['total']
    index_of_end = {int(p): s for s, p in enumerate(layout['ends'])}
    seen, moved = set(), 0
    for rows, g0, per_cutoff in expected:
        if per_cutoff is None:
            assert all(layout['snap_off'][p] < 0 for p in rows)      # a type outside 1..4 is never evaluated
            continue
        above = []
        for k in range(100, -1, -1):
            m = per_cutoff[k]
            if not m:
                continue
            end = rows[len(m) - 1]
            assert end in index_of_end, f'no snapshot ends at prediction {end} (cutoff {k})'
            s = index_of_end[end]
            assert layout['k_lo'][s] <= k <= layout['k_hi'][s] and layout['group_start'][end] == rows[0]
            off = int(layout['snap_off'][end])
            got = snaps[off:off + len(m)].tolist()
            assert got == [g0 + c if c >= 0 else -1 for c in m], f'group at prediction {rows[0]}, cutoff {k}'
            if s not in seen:
                moved += any(a != b for a, b in zip(above, m))
                above = m
            seen.add(s)
    assert len(seen) == len(layout['ends'])
    return len(seen), moved


def _scene_of_generated_groups(seed=0):
    """the groups of hungarian_ref.generated_groups packed into frames with mixed types: threshold 0.7 -> vehicle,
    0.5 -> pedestrian, 0.1 -> sign or cyclist; a frame holds at most one group per type.  Every frame also gets
    predictions and ground truth that must not take part: overlap_with_nlz, ignored (0 lidar points), degenerate boxes,
    an unknown type.  File order is shuffled."""
    rng = np.random.default_rng(seed)
    frames = []             # per frame {type: group}
    for grp in H.generated_groups(seed):
        types = {0.7: (1,), 0.5: (2,), 0.1: (3, 4)}[grp[3]]
        for fr in frames:
            free = [t for t in types if t not in fr]
            if free:
                fr[free[0]] = grp
                break
        else:
            frames.append({types[0]: grp})
    preds, gts = [], []
    mk = R.make_object
    for f, fr in enumerate(frames):
        for t, (name, pds, gs, thr, scores) in fr.items():
            preds += [mk(b, t, s, 'seg', f) for b, s in zip(pds, scores)]
            gts += [mk(b, t, 1.0, 'seg', f, points=int(rng.choice([3, 40])), level=int(rng.choice([0, 2]))) for b in gs]
            if pds and gs:
                preds.append(mk(pds[0], t, 0.99, 'seg', f, nlz=True))
                gts.append(mk(gs[0], t, 1.0, 'seg', f, points=0))
                preds.append(mk(gs[0][:3] + [0.0] + gs[0][4:], t, 0.98, 'seg', f))
                gts.append(mk(pds[0][:4] + [float('nan')] + pds[0][5:], t, 1.0, 'seg', f))
                preds.append(mk(gs[0], 5, 0.97, 'seg', f))
                gts.append(mk(pds[0], 0, 1.0, 'seg', f))
    preds = [preds[i] for i in rng.permutation(len(preds))]
    gts = [gts[i] for i in rng.permutation(len(gts))]
    return preds, gts, len(frames)


GENERATED_THRESHOLDS = (0.0, 0.7, 0.5, 0.1, 0.1)


def test_every_snapshot_equals_the_restatement_on_the_generated_groups():
    preds, gts, n_frames = _scene_of_generated_groups()
    assert n_frames >= 5
    pk, snaps, layout = _assign(preds, gts, GENERATED_THRESHOLDS)
    ious = _kernel_ious(pk)
    expected = _expected_per_cutoff(pk, ious, GENERATED_THRESHOLDS)
    n, moved = _compare_snapshots(pk, snaps, layout, expected)
    print(f'{len(preds)} predictions, {len(gts)} ground truth, {n_frames} frames, {len(ious)} overlapping pairs, '
          f'{n} snapshots ({layout["total"]} words), {moved} snapshots moved an earlier partner')
    assert n > 100 and moved > 20
    assert max(len(rows) for rows, _, m in expected if m is not None) >= 200
    # several workspace chunks in one call, and a second call: the same bytes
    _, snaps2, layout2 = _assign(preds, gts, GENERATED_THRESHOLDS, workspace_budget=64 << 10)
    assert torch.equal(snaps, snaps2) and np.array_equal(layout['snap_off'], layout2['snap_off'])
    _, snaps3, _ = _assign(preds, gts, GENERATED_THRESHOLDS)
    assert torch.equal(snaps, snaps3)


def test_every_snapshot_equals_the_restatement_on_many_small_frames():
    """1 500 frames of 0 .. 12 predictions and 0 .. 10 ground-truth boxes of two types, thresholds lowered so that
    predictions compete, in one call and in many chunks"""
    rng = np.random.default_rng(11)
    preds, gts = [], []
    for f in range(1500):
        p, g = R.random_frame(rng, int(rng.integers(0, 13)), int(rng.integers(0, 11)), ts=f, types=(1, 2), extent=6.0)
        for o in p:
            o['score'] = float(np.float32(round(o['score'] * 20) / 20))
        preds += p
        gts += g
    thr = (0.0, 0.3, 0.2, 0.5, 0.5)
    pk, snaps, layout = _assign(preds, gts, thr)
    n, moved = _compare_snapshots(pk, snaps, layout, _expected_per_cutoff(pk, _kernel_ious(pk), thr))
    print(f'{n} snapshots compared, {moved} moved an earlier partner')
    assert n > 1000 and moved > 5
    _, snaps2, _ = _assign(preds, gts, thr, workspace_budget=4 << 10)
    assert torch.equal(snaps, snaps2)


def _shifted(dx, yaw=0.0):
    return [30.0 + dx, -20.0, 1.0, 4.0, 2.0, 1.5, yaw]      # IoU with the unshifted box: (4 - |dx|) / (4 + |dx|)


def _partners(preds, gts):
    """-> per cutoff k {file index of the prediction: file index of its ground-truth box or -1} under the Hungarian matcher"""
    pk, snaps, layout = _assign(preds, gts)
    snaps = snaps.cpu().numpy()
    out = [dict() for _ in range(101)]
    for s, end in enumerate(layout['ends']):
        gs, off = int(layout['group_start'][end]), int(layout['snap_off'][end])
        for k in range(int(layout['k_lo'][s]), int(layout['k_hi'][s]) + 1):
            for r in range(end - gs + 1):
                c = int(snaps[off + r])
                out[k][int(pk['pd_order'][gs + r])] = int(pk['gt_order'][c]) if c >= 0 else -1
    return out, pk


def test_hand_example_two_boxes_three_edges():
    """g1, g2; A (0.9): IoU 0.80 to g1, 0.75 to g2; B (0.8): 0.72 to g1 only.  Score-first: A-g1, B unmatched.
    Hungarian at cutoffs <= 0.8: A-g2, B-g1 (750 + 720 > 800); between 0.8 and 0.9 A is alone and takes g1."""
    from objectcentricocccompletion_amd import waymo_metrics as M
    mk = R.make_object
    d80, d75, d72 = 4 * 0.20 / 1.80, 4 * 0.25 / 1.75, 4 * 0.28 / 1.72
    gts = [mk(_shifted(0.0), 1, points=20), mk(_shifted(d80 + d75), 1, points=20)]
    preds = [mk(_shifted(d80), 1, 0.9), mk(_shifted(-d72), 1, 0.8)]
    preds[0]['score'], preds[1]['score'] = 0.9, 0.8      # (make_object rounds scores to float32: 0.9 would fall below 90 / 100)
    partners, pk = _partners(preds, gts)
    ious = _kernel_ious(pk)
    by_file = {(int(pk['pd_order'][p]), int(pk['gt_order'][g])): v for (p, g), v in ious.items()}
    assert 0.79 < by_file[(0, 0)] < 0.81 and 0.74 < by_file[(0, 1)] < 0.76 and 0.71 < by_file[(1, 0)] < 0.73
    assert by_file.get((1, 1), 0.0) < 0.5
    for k in range(101):
        exp = {} if k > 90 else {0: 0} if k > 80 else {0: 1, 1: 0}
        assert partners[k] == exp, k
    assert partners[85][0] != partners[80][0]            # A's partner changes between the two cutoffs
    first, ap_first = M.detection_metrics(preds, gts)
    hung, ap_hung = M.detection_metrics(preds, gts, matcher='hungarian')
    # score-first: one true positive of two (recall 1/2 at precision 1); Hungarian reaches recall 1 at precision 1
    assert ap_first['Vehicle/L1 mAP'] == pytest.approx(0.5, abs=1e-12)
    assert ap_hung['Vehicle/L1 mAP'] == pytest.approx(1.0, abs=1e-12)
    assert 'score-first greedy matcher instead' in first and 'score-first' not in hung
    assert 'Hungarian matcher per score cutoff' in hung and 'recall-delta' in hung and 'not been measured' in hung


def test_hand_example_duplicates_of_one_box():
    """one box; A (0.9): IoU 0.72, heading flipped by pi (the same footprint, heading accuracy 0); B (0.8): IoU 0.90,
    heading exact.  Score-first keeps A at every cutoff; Hungarian hands the box to B from cutoff 0.8 down.  One true
    positive per cutoff either way: equal mAP, different mAPH."""
    from objectcentricocccompletion_amd import waymo_metrics as M
    mk = R.make_object
    gts = [mk(_shifted(0.0), 1, points=20)]
    preds = [mk(_shifted(4 * 0.28 / 1.72, math.pi), 1, 0.9), mk(_shifted(4 * 0.10 / 1.90), 1, 0.8)]
    preds[0]['score'], preds[1]['score'] = 0.9, 0.8      # (make_object rounds scores to float32: 0.9 would fall below 90 / 100)
    partners, pk = _partners(preds, gts)
    ious = {int(pk['pd_order'][p]): v for (p, g), v in _kernel_ious(pk).items()}
    assert 0.71 < ious[0] < 0.73 and 0.89 < ious[1] < 0.91
    for k in range(101):
        assert partners[k] == ({} if k > 90 else {0: 0} if k > 80 else {0: -1, 1: 0}), k
    _, ap_first = M.detection_metrics(preds, gts)
    _, ap_hung = M.detection_metrics(preds, gts, matcher='hungarian')
    assert ap_first['Vehicle/L1 mAP'] == ap_hung['Vehicle/L1 mAP'] == pytest.approx(1.0, abs=1e-12)
    assert ap_first['Vehicle/L1 mAPH'] == pytest.approx(0.0, abs=1e-12)
    # Hungarian, cutoffs <= 0.8: B is the true positive (heading accuracy 1), A a false positive: recall 1 at precision 1/2
    assert ap_hung['Vehicle/L1 mAPH'] == pytest.approx(0.5, abs=1e-12)
    assert ap_first['Vehicle/L1 mAPH'] != ap_hung['Vehicle/L1 mAPH']


def _table_per_cutoff(preds, gts, matches):
    """waymo_metrics_ref.table with a matching per cutoff: matches[k][i] is the ground-truth file index (or -1) of
    prediction i at cutoff k / 100"""
    out = {}
    breakdowns = [(f'OBJECT_TYPE_TYPE_{R.TYPE_NAMES[t]}', t, None) for t in (1, 2, 3, 4)]
    breakdowns += [(f'RANGE_TYPE_{R.TYPE_NAMES[t]}_{R.RANGE_NAMES[rb]}', t, rb) for t in (1, 2, 3, 4) for rb in range(3)]
    levels = [R.gt_level(g) for g in gts]
    p_bin, g_bin = [R._range_bin(p) for p in preds], [R._range_bin(g) for g in gts]
    for name, t, rb in breakdowns:
        live = [i for i, p in enumerate(preds) if not p.get('overlap_with_nlz', False) and p['type'] == t]
        for lvl in (1, 2):
            counted = lambda j: levels[j] == 1 or (lvl == 2 and levels[j] == 2)
            n_gt = sum(1 for j, g in enumerate(gts) if g['type'] == t and counted(j) and (rb is None or g_bin[j] == rb))
            pts_ap, pts_aph = [], []
            for k in range(101):
                tp = fp = 0
                tph = 0.0
                for i in live:
                    if not preds[i]['score'] >= k / 100:
                        continue
                    j = matches[k][i]
                    if j < 0:
                        if rb is None or p_bin[i] == rb:
                            fp += 1
                    elif counted(j) and (rb is None or g_bin[j] == rb):
                        tp += 1
                        tph += R._heading_accuracy(preds[i], gts[j])
                if n_gt == 0 or tp + fp == 0:
                    continue
                fn = n_gt - tp
                pts_ap.append((tp / (tp + fn), tp / (tp + fp)))
                pts_aph.append((tph / (tp + fn), tph / (tp + fp)))
            out[f'{name}_LEVEL_{lvl}'] = (R._ap(pts_ap), R._ap(pts_aph)) if n_gt else (0.0, 0.0)
    return out


def _scene_with_duplicates(rng):
    """frames of all four types in two segments; a third of the ground-truth boxes get two more predictions, the worse
    one (and sometimes a heading flip) with the higher score"""
    preds, gts = [], []
    for f in range(16):
        p, g = R.random_frame(rng, int(rng.integers(10, 40)), int(rng.integers(8, 30)), ctx=f'segment-{f % 2}', ts=f)
        for o in g[::3]:
            b = R.box_of(o)
            worse, better = list(b), list(b)
            worse[0] += 0.07 * b[3]
            worse[6] += math.pi if rng.random() < 0.5 else 0.05
            better[0] += 0.01 * b[3]
            f32 = lambda v: [float(np.float32(x)) for x in v]
            p.append(R.make_object(f32(worse), o['type'], rng.uniform(0.6, 1.0), o['context_name'], f))
            p.append(R.make_object(f32(better), o['type'], rng.uniform(0.1, 0.6), o['context_name'], f))
        preds += p
        gts += g
    preds = [preds[i] for i in rng.permutation(len(preds))]
    gts = [gts[i] for i in rng.permutation(len(gts))]
    return preds, gts


def test_whole_metric_equals_the_table_of_the_restatement():
    from objectcentricocccompletion_amd import waymo_io as W
    from objectcentricocccompletion_amd import waymo_metrics as M
    preds, gts = _scene_with_duplicates(np.random.default_rng(5))
    assert {R.gt_level(g) for g in gts} == {0, 1, 2} and any(p['overlap_with_nlz'] for p in preds)
    pk, snaps, layout = _assign(preds, gts)
    expected = _expected_per_cutoff(pk, _kernel_ious(pk), SHIPPED)
    _compare_snapshots(pk, snaps, layout, expected)
    matches = [[-1] * len(preds) for _ in range(101)]
    for rows, g0, per_cutoff in expected:
        for k in range(101):
            for r, c in enumerate(per_cutoff[k] if per_cutoff else []):
                if c >= 0:
                    matches[k][int(pk['pd_order'][rows[r]])] = int(pk['gt_order'][g0 + c])
    tab = _table_per_cutoff(preds, gts, matches)
    exp = R.ap_dict(tab)
    text, got = M.detection_metrics(preds, gts, matcher='hungarian')
    assert got == W.parse_detection_metrics(text) and set(got) == set(exp)
    worst = max(abs(got[k] - exp[k]) for k in exp)
    print(f'largest |ap_dict difference| {worst:.3e}; Vehicle/L1 mAP {exp["Vehicle/L1 mAP"]:.6f} mAPH {exp["Vehicle/L1 mAPH"]:.6f}')
    assert worst <= 1e-12
    lines = {l.split(':')[0]: l for l in text.splitlines() if not l.startswith('#')}
    assert list(lines) == list(tab)
    for k, (a, h) in tab.items():
        assert float(lines[k].split('mAP ')[1].split(']')[0]) == pytest.approx(a, abs=1e-12), k
        assert float(lines[k].split('mAPH ')[1].split(']')[0]) == pytest.approx(h, abs=1e-12), k
    assert min(exp[f'{c}/L{l} mAP'] for c in ('Vehicle', 'Pedestrian', 'Sign', 'Cyclist') for l in (1, 2)) > 0.01
    # the two matchers give different tables on this scene, so the comparison above cannot pass on the score-first path
    text_first, first = M.detection_metrics(preds, gts, matcher='score_first')
    differing = [k for k in exp if abs(first[k] - got[k]) > 1e-6]
    print(f'{len(differing)} of {len(exp)} ap_dict entries differ between the matchers, e.g. {differing[:3]}')
    assert len(differing) >= 4 and any('mAPH' in k for k in differing)
    # the default is the score-first matcher, byte for byte
    assert M.detection_metrics(preds, gts)[0] == text_first
    # two calls: the same bytes
    assert M.detection_metrics(preds, gts, matcher='hungarian')[0] == text


def test_frame_assign_checks_its_arguments():
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd import waymo_metrics as M
    dev = _dev()
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    i32 = torch.int32
    with pytest.raises(L.OcoccError, match='float32'):
        M.frame_assign(z(1, 7, dt=torch.float64), z(1, dt=i32), z(1, dt=i32), [0, 1], z(1, 7), z(1, dt=i32), z(1, dt=i32), [0, 1], [5])
    with pytest.raises(L.OcoccError, match='offsets'):
        M.frame_assign(z(1, 7), z(1, dt=i32), z(1, dt=i32), [0, 2], z(1, 7), z(1, dt=i32), z(1, dt=i32), [0, 1], [5])
    with pytest.raises(L.OcoccError, match='pd_bucket'):
        M.frame_assign(z(1, 7), z(1, dt=i32), z(1, dt=i32), [0, 1], z(1, 7), z(1, dt=i32), z(1, dt=i32), [0, 1], [5, 5])
    with pytest.raises(L.OcoccError, match='ground-truth boxes'):
        M.frame_assign(z(1, 7), z(1, dt=i32), z(1, dt=i32), [0, 1], z(5000, 7), z(5000, dt=i32), z(5000, dt=i32), [0, 5000], [5])
    with pytest.raises(L.OcoccError, match='does not fit'):
        M.frame_assign(z(1, 7), z(1, dt=i32), z(1, dt=i32), [0, 1], z(4000, 7), z(4000, dt=i32), z(4000, dt=i32), [0, 4000], [5])
    with pytest.raises(L.OcoccError):       # CPU tensors
        M.frame_assign(torch.zeros(1, 7), z(1, dt=i32), z(1, dt=i32), [0, 1], z(1, 7), z(1, dt=i32), z(1, dt=i32), [0, 1], [5])
    snaps, layout = M.frame_assign(z(0, 7), z(0, dt=i32), z(0, dt=i32), [0], z(0, 7), z(0, dt=i32), z(0, dt=i32), [0], [])
    assert snaps.numel() == 0 and layout['total'] == 0
    with pytest.raises(ValueError):
        M.detection_metrics([], [], matcher='greedy')


def test_the_tool_takes_the_matcher(tmp_path):
    from objectcentricocccompletion_amd import waymo_io as W
    data = str(tmp_path / 'data')
    run = lambda cmd: subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    p = run([sys.executable, 'tools/make_synthetic_dataset.py', data, '--tracklets', '3', '--frames', '20'])
    assert p.returncode == 0, p.stderr[-2000:]
    gt = os.path.join(data, 'waymo_format', 'gt.bin')
    tool = os.path.join(ROOT, 'tools', 'waymo_detection_metrics.py')
    p = run([sys.executable, tool, gt, gt, '--assume-points', '--matcher', 'hungarian'])
    assert p.returncode == 0, p.stderr[-3000:]
    assert 'Hungarian matcher per score cutoff' in p.stdout and 'score-first' not in p.stdout and 'recall-delta' in p.stdout
    ap = W.parse_detection_metrics(p.stdout)
    assert ap['Vehicle/L1 mAP'] == pytest.approx(1.0, abs=1e-12) and ap['Vehicle/L2 mAPH'] == pytest.approx(1.0, abs=1e-12)
    q = run([sys.executable, tool, gt, gt, '--assume-points'])
    assert q.returncode == 0 and 'score-first greedy matcher' in q.stdout
    assert W.parse_detection_metrics(q.stdout) == ap     # perfect predictions: nothing for the matchers to disagree on
    bad = run([sys.executable, tool, gt, gt, '--matcher', 'greedy'])
    assert bad.returncode != 0 and 'invalid choice' in bad.stderr
