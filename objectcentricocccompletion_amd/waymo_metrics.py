"""Native Waymo detection metrics: what the reference gets from ``compute_detection_metrics_main`` (a compiled
waymo-open-dataset tool it calls from mmdet3d/datasets/waymo_tracklet_dataset.py:352-366 and ships no source for),
computed from two metrics.Objects files with box overlap and matching on HIP kernels (csrc/frame_match.hip).

The protocol is the one DESIGN.md states ("Native Waymo detection metrics"), in short: predictions with
overlap_with_nlz are dropped; a ground-truth object is L2 when detection_difficulty_level == 2, otherwise ignored /
L2 / L1 for 0 / 1-5 / more than 5 lidar points; types vehicle, pedestrian, sign, cyclist at IoU 0.7 / 0.5 / 0.5 / 0.5;
full 3-D IoU of 7-DoF boxes; score-first greedy matching per frame and type (equal scores by file order, equal IoU to
the lower file index); OBJECT_TYPE and RANGE ([0, 30), [30, 50), [50, +inf) of the box centre's distance: the
ground-truth box of a matched pair, its own box for an unmatched prediction) breakdowns at LEVEL_1 / LEVEL_2; 101 score
cutoffs k / 100; all-point interpolated AP, APH with heading-accuracy weighted true positives.

KNOWN DEPARTURES from the official tool: (1) the tool's default matcher is Hungarian, this is its score-first
alternative -- the two differ only where one ground-truth box has several predictions above threshold; (2) the tool's
recall-delta point insertion is not reproduced.  Nobody has measured the difference to the official numbers: these are
NOT claimed to equal them.  matcher='hungarian' replaces (1) by our reading of the tool's default matcher (DESIGN 3.10
rule 4b: per score cutoff the one-to-one matching of maximum total overlap, overlaps quantised to 1/1000, ties fixed by
the insertion algorithm; frame_assign); the tool's source is not available, so that reading cannot be checked, (2) and
the last sentence stand.

Division of work: grouping, sorting and packing on the host (numpy); overlaps and matching on the device (two launches
per workspace chunk, whatever the number of frames); counts and curves in float64 on the host from the match indices
and the files' double headings, so that the metric is exactly reproducible."""
import sys

import numpy as np
import torch

from . import _lib as L
from . import waymo_io

TYPES = ((1, 'VEHICLE'), (2, 'PEDESTRIAN'), (3, 'SIGN'), (4, 'CYCLIST'))
IOU_THRESHOLDS = (0.0, 0.7, 0.5, 0.5, 0.5)          # by Waymo type number (entry 0: TYPE_UNKNOWN, never evaluated)
RANGES = (('[0, 30)', 0.0, 30.0), ('[30, 50)', 30.0, 50.0), ('[50, +inf)', 50.0, np.inf))
NUM_CUTOFFS = 101
MAX_FRAME_GT = 4096                                  # one bit of a 64-bit lane register per ground-truth box
WORKSPACE_BUDGET = 256 << 20                         # bytes of overlap matrix per call of the kernels
ASSIGN_LDS_BYTES = 64 << 10                          # LDS of one wave of the assignment kernel (frame_assign)
MATCHERS = ('score_first', 'hungarian')
CURVES_BLOCK_WORDS = 4 << 20                         # snapshot entries per block of the per-cutoff curves (host)
IGNORED, LEVEL_1, LEVEL_2 = 0, 1, 2

HEADER = ('# native Waymo detection metrics (objectcentricocccompletion_amd.waymo_metrics, HIP matching kernels)\n'
          '# departures from compute_detection_metrics_main: score-first greedy matcher instead of its default '
          'Hungarian one; no recall-delta point insertion\n'
          '# the difference to the official numbers has not been measured: do not report these as official\n')

HEADER_HUNGARIAN = ('# native Waymo detection metrics (objectcentricocccompletion_amd.waymo_metrics, HIP matching kernels)\n'
                    '# Hungarian matcher per score cutoff on overlaps quantised to 1/1000 (our reading of the tool\'s default; its '
                    'source is not available); departure from compute_detection_metrics_main: no recall-delta point insertion\n'
                    '# the difference to the official numbers has not been measured: do not report these as official\n')

_FIELDS = ('center_x', 'center_y', 'center_z', 'length', 'width', 'height', 'heading')


# ------------------------------------------------------------------------------------------------ device operator
def _checked(name, pd_boxes, pd_type, pd_eligible, pd_offsets, gt_boxes, gt_type, gt_eligible, gt_offsets):
    """the argument checks of frame_match / frame_assign -> (po, go, P, G, F)"""
    L.require_device(pd_boxes, pd_type, pd_eligible, gt_boxes, gt_type, gt_eligible)
    po, go = np.asarray(pd_offsets, dtype=np.int64), np.asarray(gt_offsets, dtype=np.int64)
    P, G, F = pd_boxes.size(0), gt_boxes.size(0), len(po) - 1
    for nm, b, n in (('pd', pd_boxes, P), ('gt', gt_boxes, G)):
        if b.dim() != 2 or b.size(1) != 7 or b.dtype != torch.float32:
            raise L.OcoccError(f'{name}: {nm}_boxes must be [N, 7] float32, got {tuple(b.shape)} {b.dtype}')
    for nm, t, n in (('pd_type', pd_type, P), ('pd_eligible', pd_eligible, P), ('gt_type', gt_type, G),
                     ('gt_eligible', gt_eligible, G)):
        if t.dtype != torch.int32 or tuple(t.shape) != (n,):
            raise L.OcoccError(f'{name}: {nm} must be [{n}] int32, got {tuple(t.shape)} {t.dtype}')
    if F < 0 or len(go) != F + 1 or po[0] != 0 or go[0] != 0 or po[-1] != P or go[-1] != G or (np.diff(po) < 0).any() \
            or (np.diff(go) < 0).any():
        raise L.OcoccError(f'{name}: offsets must start at 0, not decrease and end at the box counts')
    if P * 7 > 2 ** 31 - 1 or G * 7 > 2 ** 31 - 1:
        raise L.OcoccError(f'{name}: too many boxes for 32-bit indices')
    return po, go, P, G, F


def _chunks(name, po, go, workspace_budget):
    """-> (n_gt per frame, pair_off [F + 1], chunk boundaries: as many whole frames as fit the budget, at least one)"""
    F = len(po) - 1
    n_gt = np.diff(go)
    if int(n_gt.max()) > MAX_FRAME_GT:
        raise L.OcoccError(f'{name}: a frame has {int(n_gt.max())} ground-truth boxes, the kernel takes {MAX_FRAME_GT}')
    pair_off = np.zeros(F + 1, dtype=np.int64)
    np.cumsum(np.diff(po) * n_gt, out=pair_off[1:])
    budget_pairs = max(int(workspace_budget) // 4, 1)
    bounds, f0 = [0], 0
    while f0 < F:
        f1 = int(np.searchsorted(pair_off, pair_off[f0] + budget_pairs, side='right')) - 1
        f1 = min(max(f1, f0 + 1), F)
        bounds.append(f1)
        f0 = f1
    return n_gt, pair_off, bounds


def _run_chunks(name, export, tensors, po, go, iou_thresholds, workspace_budget, extra):
    """what frame_match and frame_assign share after their checks: contiguous inputs, the offsets and thresholds on the
    device, the workspace of the largest chunk, then one call of ``export`` per chunk.  extra(a, b, n_gt, n_pd) -> the
    arguments of the export between max_frame_gt and the workspace, for the frames [a, b)."""
    pd_boxes, pd_type, pd_eligible, gt_boxes, gt_type, gt_eligible = (t.contiguous() for t in tensors)
    dev, P, G, F = pd_boxes.device, pd_boxes.size(0), gt_boxes.size(0), len(po) - 1
    n_gt, pair_off, bounds = _chunks(name, po, go, workspace_budget)
    n_pd = np.diff(po)
    calls = [(a, b, extra(a, b, n_gt, n_pd)) for a, b in zip(bounds, bounds[1:])]     # (raises before anything is launched)
    offs = torch.from_numpy(np.concatenate([po, go]).astype(np.int32)).to(dev)
    po_dev, go_dev = offs[:F + 1], offs[F + 1:]
    pair_dev = torch.from_numpy(pair_off).to(dev)
    thr = (L.c_f32 * 5)(*[float(v) for v in iou_thresholds])
    ws_bytes = max(int(L.lib.ococc_frame_match_workspace_bytes(int(pair_off[b] - pair_off[a])))
                   for a, b in zip(bounds, bounds[1:]))
    ws = L.workspace(ws_bytes, dev)
    for a, b, more in calls:
        head, tail = more
        L.check(export(
            L.ptr(pd_boxes), L.ptr(pd_type), L.ptr(pd_eligible), L.ptr(po_dev), P, L.ptr(gt_boxes), L.ptr(gt_type),
            L.ptr(gt_eligible), L.ptr(go_dev), G, L.ptr(pair_dev), a, b, int(pair_off[a]), int(pair_off[b]),
            int(n_gt[a:b].max()), *head, thr, *tail, L.ptr(ws), ws_bytes, L.stream()), name)


def frame_match(pd_boxes, pd_type, pd_eligible, pd_offsets, gt_boxes, gt_type, gt_eligible, gt_offsets,
                iou_thresholds=IOU_THRESHOLDS, workspace_budget=WORKSPACE_BUDGET):
    """ococc_frame_match_f32.  pd_boxes [P, 7] f32 (centre x, y, z, length, width, height, heading) grouped by frame and
    sorted inside a frame by (type, descending score, file order), pd_type / pd_eligible [P] int32, device tensors;
    pd_offsets: F + 1 ints on the HOST; gt_* the same for the ground truth, grouped by frame in file order.
    -> (match_gt [P] int32: index into gt_boxes or -1, match_iou [P] f32), device tensors.  The frames are handled in
    chunks whose overlap matrices fit ``workspace_budget`` bytes (a single larger frame gets what it needs): two launches
    per chunk, none per frame."""
    po, go, P, G, F = _checked('frame_match', pd_boxes, pd_type, pd_eligible, pd_offsets, gt_boxes, gt_type, gt_eligible,
                               gt_offsets)
    dev = pd_boxes.device
    match_gt = torch.full((P,), -1, dtype=torch.int32, device=dev)
    match_iou = torch.zeros((P,), dtype=torch.float32, device=dev)
    if F == 0 or P == 0:
        return match_gt, match_iou
    _run_chunks('frame_match', L.lib.ococc_frame_match_f32, (pd_boxes, pd_type, pd_eligible, gt_boxes, gt_type, gt_eligible),
                po, go, iou_thresholds, workspace_budget, lambda a, b, n_gt, n_pd: ((), (L.ptr(match_gt), L.ptr(match_iou))))
    return match_gt, match_iou


def cutoff_buckets(scores):
    """the number of cutoffs k / 100 a prediction is part of: score >= k / 100  <=>  k < bucket"""
    return np.searchsorted(np.arange(NUM_CUTOFFS) / 100.0, np.asarray(scores, dtype=np.float64), side='right')


def snapshot_layout(pd_offsets, pd_type, pd_bucket):
    """Where frame_assign writes its per-cutoff matchings.  pd_offsets [F + 1], pd_type [P], pd_bucket [P] (cutoff_buckets
    of the scores) on the host, in the packed order; a (frame, type) group is a run of equal type inside a frame, and its
    buckets must not increase.  A snapshot ends at the last prediction of every run of equal bucket >= 1 in a group of
    type 1..4 (a bucket of 0 is part of no cutoff) and holds one int32 per prediction of the group up to that one;
    snapshots follow each other in the order of the predictions they end at.
    -> dict: snap_off [P] int64 (-1: no snapshot ends here), group_start [P] int64, ends [S] (the predictions snapshots
    end at), k_lo / k_hi [S] (the snapshot is the matching of the cutoffs k_lo .. k_hi), total (int32 words)."""
    po = np.asarray(pd_offsets, dtype=np.int64)
    ty, bk = np.asarray(pd_type, dtype=np.int64), np.asarray(pd_bucket, dtype=np.int64)
    P = len(ty)
    if len(bk) != P or len(po) < 1 or po[0] != 0 or po[-1] != P or (np.diff(po) < 0).any():
        raise L.OcoccError('snapshot_layout: pd_type and pd_bucket must be [P], pd_offsets must run from 0 to P')
    if P == 0:
        z = np.zeros(0, np.int64)
        return dict(snap_off=z, group_start=z, ends=z, k_lo=z, k_hi=z, total=0)
    frame = np.repeat(np.arange(len(po) - 1), np.diff(po))
    first = np.ones(P, dtype=bool)                       # first prediction of its (frame, type) group
    first[1:] = (frame[1:] != frame[:-1]) | (ty[1:] != ty[:-1])
    if (~first[1:] & (bk[1:] > bk[:-1])).any():
        raise L.OcoccError('snapshot_layout: the cutoff buckets of a (frame, type) group must not increase')
    group_start = np.maximum.accumulate(np.where(first, np.arange(P), 0))
    last = np.ones(P, dtype=bool)                        # last prediction of its run of equal (group, bucket)
    last[:-1] = first[1:] | (bk[1:] != bk[:-1])
    ends = np.nonzero(last & (bk >= 1) & (ty >= 1) & (ty <= 4))[0]
    lens = ends - group_start[ends] + 1
    snap_off = np.full(P, -1, dtype=np.int64)
    snap_off[ends] = np.cumsum(lens) - lens
    # the next snapshot of the same group serves the lower cutoffs from its own bucket down
    k_lo = np.zeros(len(ends), dtype=np.int64)
    same = group_start[ends[1:]] == group_start[ends[:-1]]
    k_lo[:-1] = np.where(same, bk[ends[1:]], 0)
    return dict(snap_off=snap_off, group_start=group_start, ends=ends, k_lo=k_lo, k_hi=bk[ends] - 1, total=int(lens.sum()))


def frame_assign(pd_boxes, pd_type, pd_eligible, pd_offsets, gt_boxes, gt_type, gt_eligible, gt_offsets, pd_bucket=None,
                 iou_thresholds=IOU_THRESHOLDS, workspace_budget=WORKSPACE_BUDGET, pd_type_host=None, layout=None):
    """ococc_frame_assign_i32: the maximum-total-overlap (Hungarian) matching of every (frame, type) group at every score
    cutoff (DESIGN 3.10 rule 4b).  Arguments as frame_match, plus pd_bucket: [P] ints on the HOST, cutoff_buckets of the
    scores in the packed order (pd_type_host: pd_type on the host, if the caller has it; otherwise it is copied back);
    or layout: snapshot_layout(pd_offsets, pd_type, pd_bucket) made by the caller.
    -> (snapshots: int32 device tensor, layout).  snapshots[layout['snap_off'][p] + r] is the index into gt_boxes (or -1)
    of the partner of prediction layout['group_start'][p] + r in the matching of the cutoffs layout['k_lo'] ..
    layout['k_hi'] of the snapshot that ends at p.  Chunks as in frame_match: two launches per chunk."""
    po, go, P, G, F = _checked('frame_assign', pd_boxes, pd_type, pd_eligible, pd_offsets, gt_boxes, gt_type, gt_eligible,
                               gt_offsets)
    dev = pd_boxes.device
    if layout is None:
        if pd_bucket is None:
            raise L.OcoccError('frame_assign: pd_bucket or layout is needed')
        ty = pd_type.cpu().numpy() if pd_type_host is None else np.asarray(pd_type_host)
        if len(np.asarray(pd_bucket)) != P or len(ty) != P:
            raise L.OcoccError(f'frame_assign: pd_bucket and pd_type_host must be [{P}]')
        layout = snapshot_layout(po, ty, pd_bucket)
    elif len(layout['snap_off']) != P:
        raise L.OcoccError(f'frame_assign: the layout is for {len(layout["snap_off"])} predictions, not {P}')
    snapshots = torch.full((layout['total'],), -1, dtype=torch.int32, device=dev)
    if F == 0 or P == 0:
        return snapshots, layout
    pad = lambda n: (int(n) + 63) // 64 * 64
    snap_dev = torch.from_numpy(np.ascontiguousarray(layout['snap_off'], dtype=np.int64)).to(dev)

    def extra(a, b, n_gt, n_pd):
        if 18 * pad(n_gt[a:b].max()) + 2 * pad(n_pd[a:b].max()) > ASSIGN_LDS_BYTES:
            raise L.OcoccError(f'frame_assign: a frame of up to {int(n_pd[a:b].max())} predictions and {int(n_gt[a:b].max())} '
                               f'ground-truth boxes does not fit the kernel: 18 B per ground-truth box + 2 B per '
                               f'prediction (each count rounded up to 64) must fit {ASSIGN_LDS_BYTES} B')
        return (int(n_pd[a:b].max()),), (L.ptr(snap_dev), layout['total'], L.ptr(snapshots))

    _run_chunks('frame_assign', L.lib.ococc_frame_assign_i32, (pd_boxes, pd_type, pd_eligible, gt_boxes, gt_type, gt_eligible),
                po, go, iou_thresholds, workspace_budget, extra)
    return snapshots, layout


# ------------------------------------------------------------------------------------------------ host: packing
def columns(objects):
    """list of read_bin records (or an already columnar dict of arrays) -> dict of numpy arrays, one per field"""
    if isinstance(objects, dict):
        n = len(objects['score'])
        out = {k: np.asarray(v) for k, v in objects.items()}
    else:
        n = len(objects)
        out = {k: np.array([o[k] for o in objects], dtype=np.float64).reshape(n) for k in _FIELDS + ('score',)}
        out['type'] = np.array([o['type'] for o in objects], dtype=np.int64).reshape(n)
        out['frame_timestamp_micros'] = np.array([o['frame_timestamp_micros'] for o in objects], dtype=np.int64).reshape(n)
        out['context_name'] = np.array([o['context_name'] for o in objects], dtype=object).reshape(n)
        for k, dt in (('overlap_with_nlz', bool), ('detection_difficulty_level', np.int64), ('num_lidar_points_in_box', np.int64)):
            out[k] = np.array([o.get(k, 0) for o in objects], dtype=dt).reshape(n)
    for k, dt in (('overlap_with_nlz', bool), ('detection_difficulty_level', np.int64), ('num_lidar_points_in_box', np.int64)):
        if k not in out:
            out[k] = np.zeros(n, dtype=dt)
    return out


def gt_levels(difficulty, num_points, assume_points=False):
    """-> per ground-truth object IGNORED / LEVEL_1 / LEVEL_2: detection_difficulty_level == 2 is L2, otherwise 0 points
    are ignored, 1-5 L2, more L1; assume_points: a missing (0) count is L1"""
    difficulty, num_points = np.asarray(difficulty), np.asarray(num_points)
    lvl = np.where(num_points > 5, LEVEL_1, np.where(num_points >= 1, LEVEL_2, LEVEL_1 if assume_points else IGNORED))
    return np.where(difficulty == 2, LEVEL_2, lvl).astype(np.int32)


def _frame_ids(pd, gt):
    """frame number of every prediction and ground-truth object: (context_name, frame_timestamp_micros) pairs numbered
    in sorted order over both files"""
    names = np.concatenate([pd['context_name'], gt['context_name']])
    ts = np.concatenate([pd['frame_timestamp_micros'], gt['frame_timestamp_micros']]).astype(np.int64)
    if len(names) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    _, code = np.unique(names.astype(str), return_inverse=True)
    order = np.lexsort((ts, code))
    new = np.ones(len(order), dtype=bool)
    new[1:] = (code[order][1:] != code[order][:-1]) | (ts[order][1:] != ts[order][:-1])
    fid = np.empty(len(order), dtype=np.int64)
    fid[order] = np.cumsum(new) - 1
    n_pd = len(pd['score'])
    return fid[:n_pd], fid[n_pd:], int(new.sum())


def pack(pd, gt, assume_points=False):
    """columns of the two files -> the packed host arrays of frame_match plus what the curves need.  Predictions sorted
    by (frame, type, descending score, file order), ground truth by (frame, file order)."""
    pf, gf, F = _frame_ids(pd, gt)
    n_pd, n_gt = len(pf), len(gf)
    p_order = np.lexsort((np.arange(n_pd), -pd['score'], pd['type'], pf)) if n_pd else np.zeros(0, np.int64)
    g_order = np.argsort(gf, kind='stable') if n_gt else np.zeros(0, np.int64)
    level = gt_levels(gt['detection_difficulty_level'], gt['num_lidar_points_in_box'], assume_points)
    evaluated = lambda t: (t >= 1) & (t <= 4)
    box64 = lambda c, order: np.stack([c[k][order] for k in _FIELDS], 1).reshape(len(order), 7).astype(np.float64)
    out = dict(
        F=F,
        pd_boxes=box64(pd, p_order), gt_boxes=box64(gt, g_order),
        pd_type=pd['type'][p_order].astype(np.int32), gt_type=gt['type'][g_order].astype(np.int32),
        pd_score=pd['score'][p_order].astype(np.float64),
        pd_eligible=(~pd['overlap_with_nlz'][p_order].astype(bool) & evaluated(pd['type'][p_order])).astype(np.int32),
        gt_level=level[g_order],
        pd_offsets=np.searchsorted(pf[p_order], np.arange(F + 1)).astype(np.int64),
        gt_offsets=np.searchsorted(gf[g_order], np.arange(F + 1)).astype(np.int64),
        pd_order=p_order, gt_order=g_order)
    out['gt_eligible'] = ((out['gt_level'] != IGNORED) & evaluated(out['gt_type'])).astype(np.int32)
    return out


# ------------------------------------------------------------------------------------------------ host: curves
def heading_accuracy(pd_heading, gt_heading):
    d = np.mod(np.asarray(pd_heading, np.float64) - np.asarray(gt_heading, np.float64), 2 * np.pi)
    return 1.0 - np.minimum(np.abs(d), 2 * np.pi - np.abs(d)) / np.pi


def average_precision(num, tp_fp, denom_recall):
    """num [K]: the numerator of precision and recall at each cutoff (TP, or TPH), tp_fp [K]: TP + FP,
    denom_recall [K]: TP + FN.  All-point interpolated area: points with TP + FP == 0 left out, the point recall 0
    added, precision made non-increasing in recall from the right, sum of (r_i - r_{i-1}) * p_i over distinct recalls."""
    keep = tp_fp > 0
    if not keep.any() or not (denom_recall > 0).all():
        return 0.0
    p, r = num[keep] / tp_fp[keep], num[keep] / denom_recall[keep]
    rs, inv = np.unique(r, return_inverse=True)
    ps = np.zeros(len(rs))
    np.maximum.at(ps, inv, p)
    ps = np.maximum.accumulate(ps[::-1])[::-1]
    return float(np.sum(np.diff(np.concatenate([[0.0], rs])) * ps))


def _range_bin(boxes):
    d = np.sqrt(boxes[:, 0] ** 2 + boxes[:, 1] ** 2 + boxes[:, 2] ** 2)
    return np.where(d < 30.0, 0, np.where(d < 50.0, 1, 2))


def curves(pk, match_gt=None, per_cutoff=None):
    """packed arrays + match indices -> {breakdown name: (AP, APH)} in the tool's order.  match_gt [P]: one matching that
    serves every cutoff (the score-first matcher); or per_cutoff = (snapshots, layout) as frame_assign returns them
    (snapshots on the host): the matching of each cutoff on its own (matcher='hungarian')."""
    if per_cutoff is not None:
        return _curves_per_cutoff(pk, np.asarray(per_cutoff[0]), per_cutoff[1])
    match_gt = np.asarray(match_gt, dtype=np.int64)
    cut = np.arange(NUM_CUTOFFS) / 100.0
    elig = pk['pd_eligible'] != 0
    matched = match_gt >= 0
    mg = np.where(matched, match_gt, 0)
    # the number of cutoffs a prediction is part of: score >= k / 100  <=>  k < n_cut
    n_cut = np.searchsorted(cut, pk['pd_score'], side='right')
    tp_level = np.where(matched, pk['gt_level'][mg] if len(pk['gt_level']) else 0, 0)
    ha = np.where(matched, heading_accuracy(pk['pd_boxes'][:, 6], pk['gt_boxes'][mg, 6] if len(pk['gt_boxes']) else 0.0), 0.0)
    p_bin = np.where(matched, _range_bin(pk['gt_boxes'][mg]) if len(pk['gt_boxes']) else 0, _range_bin(pk['pd_boxes']))
    g_bin = _range_bin(pk['gt_boxes'])

    def at_cutoffs(sel, weights=None):
        """[K]: sum (of weights) over the selected predictions with score >= cutoff k"""
        h = np.bincount(n_cut[sel], weights=None if weights is None else weights[sel], minlength=NUM_CUTOFFS + 1)
        return (h.sum() - np.cumsum(h))[:NUM_CUTOFFS].astype(np.float64)   # predictions with n_cut > k

    out = {}

    def one(name, t, rb):
        for lvl in (LEVEL_1, LEVEL_2):
            g_sel = (pk['gt_type'] == t) & (pk['gt_level'] != IGNORED) & ((pk['gt_level'] == LEVEL_1) | (lvl == LEVEL_2))
            p_sel = elig & (pk['pd_type'] == t)
            if rb is not None:
                g_sel, p_sel = g_sel & (g_bin == rb), p_sel & (p_bin == rb)
            n_g = int(g_sel.sum())
            tp_sel = p_sel & matched & ((tp_level == LEVEL_1) | (lvl == LEVEL_2))
            tp, fp = at_cutoffs(tp_sel), at_cutoffs(p_sel & ~matched)
            tph = at_cutoffs(tp_sel, ha)
            key = f'{name}_LEVEL_{lvl}'
            if n_g == 0:
                out[key] = (0.0, 0.0)
                continue
            fn = n_g - tp
            out[key] = (average_precision(tp, tp + fp, tp + fn), average_precision(tph, tp + fp, tp + fn))

    for t, tname in TYPES:
        one(f'OBJECT_TYPE_TYPE_{tname}', t, None)
    for t, tname in TYPES:
        for rb, (rname, _, _) in enumerate(RANGES):
            one(f'RANGE_TYPE_{tname}_{rname}', t, rb)
    return out


def _curves_per_cutoff(pk, snapshots, layout, block_words=CURVES_BLOCK_WORDS):
    """Rules 5 and 6 with a matching per cutoff.  An entry of a snapshot is one (prediction, partner) pair that holds
    for the cutoffs k_lo .. k_hi of its snapshot; entries are binned by cell = (type, range bin, unmatched / matched to
    LEVEL_1 / matched to LEVEL_2) and added to the cutoffs they hold for by a difference array over k (counts are exact;
    the heading-weighted sums are float64).  The difference arrays are additive, so the snapshots are taken in blocks of
    about ``block_words`` entries: the temporaries are bounded by the block, not by the file."""
    K = NUM_CUTOFFS + 1
    ends, total = layout['ends'], layout['total']
    if len(snapshots) != total:
        raise L.OcoccError(f'curves: {len(snapshots)} snapshot words, the layout has {total}')
    n_gt_all = len(pk['gt_boxes'])
    g_bin = _range_bin(pk['gt_boxes'])
    own_bin = _range_bin(pk['pd_boxes'])
    gs_of = layout['group_start'][ends]
    lens = ends - gs_of + 1
    start = np.cumsum(lens) - lens
    d_count, d_heading = np.zeros(36 * K + 1), np.zeros(36 * K + 1)
    s0 = 0
    while s0 < len(ends):
        s1 = max(int(np.searchsorted(start, start[s0] + block_words, side='right')), s0 + 1)     # snapshots [s0, s1)
        n = int(start[s1 - 1] + lens[s1 - 1] - start[s0])
        sid = np.repeat(np.arange(s1 - s0), lens[s0:s1])                 # snapshot of every entry, block-local
        pidx = gs_of[s0:s1][sid] + (np.arange(n) - (start[s0:s1] - start[s0])[sid])
        part = np.asarray(snapshots[start[s0]:start[s0] + n], dtype=np.int64)
        use = pk['pd_eligible'][pidx] != 0
        sid, pidx, part = sid[use], pidx[use], part[use]
        matched = part >= 0
        mg = np.where(matched, part, 0)
        level = np.where(matched, pk['gt_level'][mg] if n_gt_all else 0, 0)
        ha = np.where(matched, heading_accuracy(pk['pd_boxes'][pidx, 6], pk['gt_boxes'][mg, 6] if n_gt_all else 0.0), 0.0)
        p_bin = np.where(matched, g_bin[mg] if n_gt_all else 0, own_bin[pidx])
        state = np.where(matched, np.where(level == LEVEL_1, 1, 2), 0)
        cell = ((pk['pd_type'][pidx].astype(np.int64) - 1) * 3 + p_bin) * 3 + state
        lo, hi = cell * K + layout['k_lo'][s0:s1][sid], cell * K + layout['k_hi'][s0:s1][sid] + 1
        d_count += np.bincount(lo, minlength=36 * K + 1) - np.bincount(hi, minlength=36 * K + 1)
        d_heading += np.bincount(lo, weights=ha, minlength=36 * K + 1) - np.bincount(hi, weights=ha, minlength=36 * K + 1)
        s0 = s1
    over = lambda d: np.cumsum(d[:36 * K].reshape(36, K), axis=1)[:, :NUM_CUTOFFS].reshape(4, 3, 3, NUM_CUTOFFS)
    count, heading = over(d_count), over(d_heading)
    out = {}

    def one(name, t, rb):
        bins = slice(None) if rb is None else slice(rb, rb + 1)
        for lvl in (LEVEL_1, LEVEL_2):
            g_sel = (pk['gt_type'] == t) & (pk['gt_level'] != IGNORED) & ((pk['gt_level'] == LEVEL_1) | (lvl == LEVEL_2))
            if rb is not None:
                g_sel = g_sel & (g_bin == rb)
            n_g = int(g_sel.sum())
            states = slice(1, 2) if lvl == LEVEL_1 else slice(1, 3)
            tp, tph = count[t - 1, bins, states].sum((0, 1)), heading[t - 1, bins, states].sum((0, 1))
            fp = count[t - 1, bins, 0].sum(0)
            key = f'{name}_LEVEL_{lvl}'
            if n_g == 0:
                out[key] = (0.0, 0.0)
                continue
            fn = n_g - tp
            out[key] = (average_precision(tp, tp + fp, tp + fn), average_precision(tph, tp + fp, tp + fn))

    for t, tname in TYPES:
        one(f'OBJECT_TYPE_TYPE_{tname}', t, None)
    for t, tname in TYPES:
        for rb, (rname, _, _) in enumerate(RANGES):
            one(f'RANGE_TYPE_{tname}_{rname}', t, rb)
    return out


def format_table(table):
    """{name: (AP, APH)} -> the tool's text layout (15 significant digits, so that parsing loses nothing that matters)"""
    return ''.join(f'{k}: [mAP {ap:.15g}] [mAPH {aph:.15g}]\n' for k, (ap, aph) in table.items())


# ------------------------------------------------------------------------------------------------ the metric
def detection_metrics(pred_objects, gt_objects, assume_points=False, device=None, timings=None, matcher='score_first'):
    """pred_objects / gt_objects: what waymo_io.read_bin returns (or columns() of it) -> (text, ap_dict): the table in
    the layout of compute_detection_metrics_main under a '#' header, and waymo_io.parse_detection_metrics of it.
    assume_points: treat a missing lidar point count as LEVEL_1 (files written without the counts), with one warning
    line.  Matching runs on ``device`` (default: the current ROCm device); there is no CPU fallback.  KNOWN DEPARTURES
    from the official tool: score-first greedy matcher instead of Hungarian, no recall-delta point insertion; the
    difference to the official numbers has not been measured.  timings: a dict that receives host_pack / kernels /
    host_curves in seconds.  matcher: 'score_first' (the default, as above) or 'hungarian': the matching of every score
    cutoff is the one of maximum total overlap among the predictions above the cutoff (DESIGN 3.10 rule 4b, our reading
    of the tool's default matcher; frame_assign), which removes the first departure and leaves the second."""
    import time
    if matcher not in MATCHERS:
        raise ValueError(f'matcher {matcher!r} is not one of {MATCHERS}')
    if not torch.cuda.is_available():
        raise L.OcoccError('waymo_native runs its matching on a ROCm device only (there is no CPU fallback)')
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    L.require_device(torch.empty(0, device=dev))
    t0 = time.perf_counter()
    pd, gt = columns(pred_objects), columns(gt_objects)
    header = HEADER if matcher == 'score_first' else HEADER_HUNGARIAN
    if assume_points:
        line = ('WARNING: --assume-points: ground-truth objects without a lidar point count are taken as LEVEL_1 '
                f'({int((gt["num_lidar_points_in_box"] == 0).sum())} of {len(gt["score"])})')
        print(line, file=sys.stderr)
        header += f'# {line}\n'
    if matcher == 'hungarian' and np.isnan(pd['score']).any():
        raise L.OcoccError(f"matcher='hungarian': {int(np.isnan(pd['score']).sum())} predictions have a NaN score; a score "
                           'cutoff has no meaning for them (the score-first matcher counts them at every cutoff)')
    pk = pack(pd, gt, assume_points)
    t1 = time.perf_counter()
    with torch.cuda.device(dev):
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(dev)
        args = (up(pk['pd_boxes'], np.float32), up(pk['pd_type'], np.int32), up(pk['pd_eligible'], np.int32),
                pk['pd_offsets'], up(pk['gt_boxes'], np.float32), up(pk['gt_type'], np.int32),
                up(pk['gt_eligible'], np.int32), pk['gt_offsets'])
        if matcher == 'score_first':
            match_gt, _ = frame_match(*args)
            match_gt = match_gt.cpu().numpy()        # (synchronises)
        else:
            snapshots, layout = frame_assign(*args, cutoff_buckets(pk['pd_score']), pd_type_host=pk['pd_type'])
            snapshots = snapshots.cpu().numpy()      # (synchronises)
    t2 = time.perf_counter()
    table = curves(pk, match_gt) if matcher == 'score_first' else curves(pk, per_cutoff=(snapshots, layout))
    text = header + format_table(table)
    t3 = time.perf_counter()
    if timings is not None:
        timings.update(host_pack=t1 - t0, kernels=t2 - t1, host_curves=t3 - t2)
    return text, waymo_io.parse_detection_metrics(text)


def evaluate_files(pred_bin, gt_bin, assume_points=False, txt_path=None, matcher='score_first'):
    """two metrics.Objects files -> ap_dict; prints the table, and writes it to ``txt_path`` when given"""
    if matcher not in MATCHERS:
        raise ValueError(f'matcher {matcher!r} is not one of {MATCHERS}')
    text, ap = detection_metrics(waymo_io.read_bin(pred_bin), waymo_io.read_bin(gt_bin), assume_points, matcher=matcher)
    print(text, end='')
    if txt_path:
        with open(txt_path, 'w') as fw:
            fw.write(text)
    return ap
