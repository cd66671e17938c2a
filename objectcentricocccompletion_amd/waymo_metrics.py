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
NOT claimed to equal them.

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
IGNORED, LEVEL_1, LEVEL_2 = 0, 1, 2

HEADER = ('# native Waymo detection metrics (objectcentricocccompletion_amd.waymo_metrics, HIP matching kernels)\n'
          '# departures from compute_detection_metrics_main: score-first greedy matcher instead of its default '
          'Hungarian one; no recall-delta point insertion\n'
          '# the difference to the official numbers has not been measured: do not report these as official\n')

_FIELDS = ('center_x', 'center_y', 'center_z', 'length', 'width', 'height', 'heading')


# ------------------------------------------------------------------------------------------------ device operator
def frame_match(pd_boxes, pd_type, pd_eligible, pd_offsets, gt_boxes, gt_type, gt_eligible, gt_offsets,
                iou_thresholds=IOU_THRESHOLDS, workspace_budget=WORKSPACE_BUDGET):
    """ococc_frame_match_f32.  pd_boxes [P, 7] f32 (centre x, y, z, length, width, height, heading) grouped by frame and
    sorted inside a frame by (type, descending score, file order), pd_type / pd_eligible [P] int32, device tensors;
    pd_offsets: F + 1 ints on the HOST; gt_* the same for the ground truth, grouped by frame in file order.
    -> (match_gt [P] int32: index into gt_boxes or -1, match_iou [P] f32), device tensors.  The frames are handled in
    chunks whose overlap matrices fit ``workspace_budget`` bytes (a single larger frame gets what it needs): two launches
    per chunk, none per frame."""
    L.require_device(pd_boxes, pd_type, pd_eligible, gt_boxes, gt_type, gt_eligible)
    po, go = np.asarray(pd_offsets, dtype=np.int64), np.asarray(gt_offsets, dtype=np.int64)
    P, G, F = pd_boxes.size(0), gt_boxes.size(0), len(po) - 1
    for name, b, n in (('pd', pd_boxes, P), ('gt', gt_boxes, G)):
        if b.dim() != 2 or b.size(1) != 7 or b.dtype != torch.float32:
            raise L.OcoccError(f'frame_match: {name}_boxes must be [N, 7] float32, got {tuple(b.shape)} {b.dtype}')
    for name, t, n in (('pd_type', pd_type, P), ('pd_eligible', pd_eligible, P), ('gt_type', gt_type, G),
                       ('gt_eligible', gt_eligible, G)):
        if t.dtype != torch.int32 or tuple(t.shape) != (n,):
            raise L.OcoccError(f'frame_match: {name} must be [{n}] int32, got {tuple(t.shape)} {t.dtype}')
    if F < 0 or len(go) != F + 1 or po[0] != 0 or go[0] != 0 or po[-1] != P or go[-1] != G or (np.diff(po) < 0).any() \
            or (np.diff(go) < 0).any():
        raise L.OcoccError('frame_match: offsets must start at 0, not decrease and end at the box counts')
    if P * 7 > 2 ** 31 - 1 or G * 7 > 2 ** 31 - 1:
        raise L.OcoccError('frame_match: too many boxes for 32-bit indices')
    dev = pd_boxes.device
    match_gt = torch.full((P,), -1, dtype=torch.int32, device=dev)
    match_iou = torch.zeros((P,), dtype=torch.float32, device=dev)
    if F == 0 or P == 0:
        return match_gt, match_iou
    n_gt = np.diff(go)
    if int(n_gt.max()) > MAX_FRAME_GT:
        raise L.OcoccError(f'frame_match: a frame has {int(n_gt.max())} ground-truth boxes, the kernel takes {MAX_FRAME_GT}')
    pair_off = np.zeros(F + 1, dtype=np.int64)
    np.cumsum(np.diff(po) * n_gt, out=pair_off[1:])
    pd_boxes, gt_boxes = pd_boxes.contiguous(), gt_boxes.contiguous()
    pd_type, pd_eligible, gt_type, gt_eligible = (t.contiguous() for t in (pd_type, pd_eligible, gt_type, gt_eligible))
    offs = torch.from_numpy(np.concatenate([po, go]).astype(np.int32)).to(dev)
    po_dev, go_dev = offs[:F + 1], offs[F + 1:]
    pair_dev = torch.from_numpy(pair_off).to(dev)
    thr = (L.c_f32 * 5)(*[float(v) for v in iou_thresholds])
    budget_pairs = max(int(workspace_budget) // 4, 1)
    # chunk boundaries: as many whole frames as fit the budget, at least one
    bounds, f0 = [0], 0
    while f0 < F:
        f1 = int(np.searchsorted(pair_off, pair_off[f0] + budget_pairs, side='right')) - 1
        f1 = min(max(f1, f0 + 1), F)
        bounds.append(f1)
        f0 = f1
    ws_bytes = max(int(L.lib.ococc_frame_match_workspace_bytes(int(pair_off[b] - pair_off[a])))
                   for a, b in zip(bounds, bounds[1:]))
    ws = L.workspace(ws_bytes, dev)
    for a, b in zip(bounds, bounds[1:]):
        L.check(L.lib.ococc_frame_match_f32(
            L.ptr(pd_boxes), L.ptr(pd_type), L.ptr(pd_eligible), L.ptr(po_dev), P, L.ptr(gt_boxes), L.ptr(gt_type),
            L.ptr(gt_eligible), L.ptr(go_dev), G, L.ptr(pair_dev), a, b, int(pair_off[a]), int(pair_off[b]),
            int(n_gt[a:b].max()), thr, L.ptr(match_gt), L.ptr(match_iou), L.ptr(ws), ws_bytes, L.stream()), 'frame_match')
    return match_gt, match_iou


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


def curves(pk, match_gt):
    """packed arrays + match indices -> {breakdown name: (AP, APH)} in the tool's order"""
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


def format_table(table):
    """{name: (AP, APH)} -> the tool's text layout (15 significant digits, so that parsing loses nothing that matters)"""
    return ''.join(f'{k}: [mAP {ap:.15g}] [mAPH {aph:.15g}]\n' for k, (ap, aph) in table.items())


# ------------------------------------------------------------------------------------------------ the metric
def detection_metrics(pred_objects, gt_objects, assume_points=False, device=None, timings=None):
    """pred_objects / gt_objects: what waymo_io.read_bin returns (or columns() of it) -> (text, ap_dict): the table in
    the layout of compute_detection_metrics_main under a '#' header, and waymo_io.parse_detection_metrics of it.
    assume_points: treat a missing lidar point count as LEVEL_1 (files written without the counts), with one warning
    line.  Matching runs on ``device`` (default: the current ROCm device); there is no CPU fallback.  KNOWN DEPARTURES
    from the official tool: score-first greedy matcher instead of Hungarian, no recall-delta point insertion; the
    difference to the official numbers has not been measured.  timings: a dict that receives host_pack / kernels /
    host_curves in seconds."""
    import time
    if not torch.cuda.is_available():
        raise L.OcoccError('waymo_native runs its matching on a ROCm device only (there is no CPU fallback)')
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    L.require_device(torch.empty(0, device=dev))
    t0 = time.perf_counter()
    pd, gt = columns(pred_objects), columns(gt_objects)
    header = HEADER
    if assume_points:
        line = ('WARNING: --assume-points: ground-truth objects without a lidar point count are taken as LEVEL_1 '
                f'({int((gt["num_lidar_points_in_box"] == 0).sum())} of {len(gt["score"])})')
        print(line, file=sys.stderr)
        header += f'# {line}\n'
    pk = pack(pd, gt, assume_points)
    t1 = time.perf_counter()
    with torch.cuda.device(dev):
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(dev)
        match_gt, _ = frame_match(up(pk['pd_boxes'], np.float32), up(pk['pd_type'], np.int32), up(pk['pd_eligible'], np.int32),
                                  pk['pd_offsets'], up(pk['gt_boxes'], np.float32), up(pk['gt_type'], np.int32),
                                  up(pk['gt_eligible'], np.int32), pk['gt_offsets'])
        match_gt = match_gt.cpu().numpy()            # (synchronises)
    t2 = time.perf_counter()
    text = header + format_table(curves(pk, match_gt))
    t3 = time.perf_counter()
    if timings is not None:
        timings.update(host_pack=t1 - t0, kernels=t2 - t1, host_curves=t3 - t2)
    return text, waymo_io.parse_detection_metrics(text)


def evaluate_files(pred_bin, gt_bin, assume_points=False, txt_path=None):
    """two metrics.Objects files -> ap_dict; prints the table, and writes it to ``txt_path`` when given"""
    text, ap = detection_metrics(waymo_io.read_bin(pred_bin), waymo_io.read_bin(gt_bin), assume_points)
    print(text, end='')
    if txt_path:
        with open(txt_path, 'w') as fw:
            fw.write(text)
    return ap
