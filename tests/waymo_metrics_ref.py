"""Float64 restatement of the native Waymo detection metric's protocol ("Native Waymo detection metrics"),
the checker of tests/test_waymo_metrics_cpu.py and tests/test_gpu_waymo_metrics.py.  It shares no algorithm with
csrc/frame_match.hip or waymo_metrics.py: the BEV intersection is the convex hull (scipy) of (corners of A inside B) +
(corners of B inside A) + (edge crossings), in world coordinates; matching and curves are straight loops over Python
lists.  Objects are dicts as waymo_io.read_bin returns them."""
import math

import numpy as np
from scipy.spatial import ConvexHull

THRESH = {1: 0.7, 2: 0.5, 3: 0.5, 4: 0.5}
TYPE_NAMES = {1: 'VEHICLE', 2: 'PEDESTRIAN', 3: 'SIGN', 4: 'CYCLIST'}
CLASS_NAMES = {1: 'Vehicle', 2: 'Pedestrian', 3: 'Sign', 4: 'Cyclist'}
RANGE_NAMES = ('[0, 30)', '[30, 50)', '[50, +inf)')
BOX_KEYS = ('center_x', 'center_y', 'center_z', 'length', 'width', 'height', 'heading')


def box_of(o):
    return [float(o[k]) for k in BOX_KEYS]


def corners(b):
    cx, cy, l, w, h = b[0], b[1], b[3], b[4], b[6]
    c, s = math.cos(h), math.sin(h)
    return [np.array([cx + dx * c - dy * s, cy + dx * s + dy * c]) for dx, dy in
            ((l / 2, w / 2), (-l / 2, w / 2), (-l / 2, -w / 2), (l / 2, -w / 2))]      # counter-clockwise


def _inside(p, quad):
    for i in range(4):
        a, b = quad[i], quad[(i + 1) % 4]
        if (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]) < 0:
            return False
    return True


def bev_intersection(a, b):
    A, B = corners(a), corners(b)
    pts = [p for p in A if _inside(p, B)] + [p for p in B if _inside(p, A)]
    for i in range(4):
        p, r = A[i], A[(i + 1) % 4] - A[i]
        for j in range(4):
            q, s = B[j], B[(j + 1) % 4] - B[j]
            d = r[0] * s[1] - r[1] * s[0]
            if abs(d) < 1e-14:
                continue
            t = ((q - p)[0] * s[1] - (q - p)[1] * s[0]) / d
            u = ((q - p)[0] * r[1] - (q - p)[1] * r[0]) / d
            if 0 <= t <= 1 and 0 <= u <= 1:
                pts.append(p + t * r)
    if len(pts) < 3:
        return 0.0
    pts = np.unique(np.round(np.array(pts), 12), axis=0)
    if len(pts) < 3:
        return 0.0
    try:
        return float(ConvexHull(pts).volume)
    except Exception:      # all points on a line
        return 0.0


def iou3d(a, b):
    """a, b: [cx, cy, cz, length, width, height, heading]; degenerate boxes (extent <= 0, non-finite) give 0"""
    for x in (a, b):
        if not all(math.isfinite(v) for v in x) or not (x[3] > 0 and x[4] > 0 and x[5] > 0):
            return 0.0
    if math.hypot(a[0] - b[0], a[1] - b[1]) > (math.hypot(a[3], a[4]) + math.hypot(b[3], b[4])) / 2:
        return 0.0      # the circumscribed circles are apart (what keeps a 600 x 400 frame affordable in Python)
    top = min(a[2] + a[5] / 2, b[2] + b[5] / 2)
    bot = max(a[2] - a[5] / 2, b[2] - b[5] / 2)
    if top - bot <= 0:
        return 0.0
    inter = bev_intersection(a, b) * (top - bot)
    union = a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - inter
    return inter / union if union > 0 else 0.0


def gt_level(o, assume_points=False):
    """0 ignored, 1, 2"""
    if o.get('detection_difficulty_level', 0) == 2:
        return 2
    n = o.get('num_lidar_points_in_box', 0)
    if n > 5:
        return 1
    if n >= 1:
        return 2
    return 1 if assume_points else 0


def match(preds, gts, assume_points=False, iou_fn=iou3d):
    """-> per prediction (file order) the file index of the ground-truth object it takes, or -1"""
    out = [-1] * len(preds)
    frames = {}
    for i, p in enumerate(preds):
        if p.get('overlap_with_nlz', False) or p['type'] not in THRESH:
            continue
        frames.setdefault((p['context_name'], p['frame_timestamp_micros'], p['type']), ([], []))[0].append(i)
    for j, g in enumerate(gts):
        if gt_level(g, assume_points) == 0 or g['type'] not in THRESH:
            continue
        key = (g['context_name'], g['frame_timestamp_micros'], g['type'])
        if key in frames:
            frames[key][1].append(j)
    for (_, _, t), (pi, gj) in frames.items():
        taken = set()
        for i in sorted(pi, key=lambda i: (-preds[i]['score'], i)):
            best, best_j = -1.0, -1
            for j in gj:
                if j in taken:
                    continue
                v = iou_fn(box_of(preds[i]), box_of(gts[j]))
                if v >= THRESH[t] and v > best:
                    best, best_j = v, j
            if best_j >= 0:
                taken.add(best_j)
                out[i] = best_j
    return out


def _range_bin(o):
    d = math.sqrt(o['center_x'] ** 2 + o['center_y'] ** 2 + o['center_z'] ** 2)
    return 0 if d < 30 else (1 if d < 50 else 2)


def _heading_accuracy(p, g):
    d = (p['heading'] - g['heading']) % (2 * math.pi)
    return 1 - min(abs(d), 2 * math.pi - abs(d)) / math.pi


def _ap(points):
    """points: list of (recall, precision)"""
    if not points:
        return 0.0
    best = {}
    for r, p in points:
        best[r] = max(best.get(r, 0.0), p)
    rs = sorted(best)
    ps = [best[r] for r in rs]
    for i in range(len(ps) - 2, -1, -1):
        ps[i] = max(ps[i], ps[i + 1])
    area, prev = 0.0, 0.0
    for r, p in zip(rs, ps):
        area += (r - prev) * p
        prev = r
    return area


def table(preds, gts, matches, assume_points=False):
    """-> {breakdown name: (AP, APH)}"""
    out = {}
    breakdowns = [(f'OBJECT_TYPE_TYPE_{TYPE_NAMES[t]}', t, None) for t in (1, 2, 3, 4)]
    breakdowns += [(f'RANGE_TYPE_{TYPE_NAMES[t]}_{RANGE_NAMES[rb]}', t, rb) for t in (1, 2, 3, 4) for rb in range(3)]
    levels = [gt_level(g, assume_points) for g in gts]
    for name, t, rb in breakdowns:
        for lvl in (1, 2):
            counted = lambda j: levels[j] == 1 or (lvl == 2 and levels[j] == 2)
            n_gt = sum(1 for j, g in enumerate(gts) if g['type'] == t and counted(j) and (rb is None or _range_bin(g) == rb))
            pts_ap, pts_aph = [], []
            for k in range(101):
                cut = k / 100
                tp = fp = 0
                tph = 0.0
                for i, p in enumerate(preds):
                    if p.get('overlap_with_nlz', False) or p['type'] != t or not p['score'] >= cut:
                        continue
                    j = matches[i]
                    if j < 0:
                        if rb is None or _range_bin(p) == rb:
                            fp += 1
                    elif counted(j) and (rb is None or _range_bin(gts[j]) == rb):
                        tp += 1
                        tph += _heading_accuracy(p, gts[j])
                if n_gt == 0 or tp + fp == 0:
                    continue
                fn = n_gt - tp
                pts_ap.append((tp / (tp + fn), tp / (tp + fp)))
                pts_aph.append((tph / (tp + fn), tph / (tp + fp)))
            out[f'{name}_LEVEL_{lvl}'] = (_ap(pts_ap), _ap(pts_aph)) if n_gt else (0.0, 0.0)
    return out


def ap_dict(tab):
    ap = {}
    for t in (1, 2, 3, 4):
        for lvl in (1, 2):
            a, h = tab[f'OBJECT_TYPE_TYPE_{TYPE_NAMES[t]}_LEVEL_{lvl}']
            ap[f'{CLASS_NAMES[t]}/L{lvl} mAP'], ap[f'{CLASS_NAMES[t]}/L{lvl} mAPH'] = a, h
    for lvl in (1, 2):
        for m in ('mAP', 'mAPH'):
            ap[f'Overall/L{lvl} {m}'] = (ap[f'Vehicle/L{lvl} {m}'] + ap[f'Pedestrian/L{lvl} {m}'] + ap[f'Cyclist/L{lvl} {m}']) / 3
    return ap


def detection_metrics(preds, gts, assume_points=False):
    m = match(preds, gts, assume_points)
    tab = table(preds, gts, m, assume_points)
    return tab, ap_dict(tab)


# ------------------------------------------------------------------------------------------------ generators
def make_object(box, type=1, score=1.0, ctx='seg', ts=0, nlz=False, level=0, points=20, id=''):
    o = dict(zip(BOX_KEYS, [float(v) for v in box]))
    o.update(type=type, score=float(np.float32(score)), context_name=ctx, frame_timestamp_micros=ts, id=id,
             overlap_with_nlz=bool(nlz), detection_difficulty_level=level, num_lidar_points_in_box=points)
    return o


_SIZES = {1: ((3.5, 6.0), (1.6, 2.4), (1.4, 2.2)), 2: ((0.5, 1.1), (0.5, 1.0), (1.4, 2.0)),
          3: ((0.3, 0.9), (0.1, 0.4), (0.5, 1.2)), 4: ((1.4, 2.1), (0.5, 0.9), (1.4, 1.9))}


def random_frame(rng, n_pd, n_gt, ctx='seg', ts=0, types=(1, 2, 3, 4), extent=75.0):
    """One frame: ground truth spread over +-extent m, most predictions perturbed copies of a ground-truth box (some of
    them twice, so that predictions compete), the rest free.  All values are rounded to float32 first (what the kernel
    sees is then exactly what the checker sees)."""
    f32 = lambda v: [float(np.float32(x)) for x in v]
    gts, preds = [], []
    for _ in range(n_gt):
        t = int(rng.choice(types))
        (l0, l1), (w0, w1), (h0, h1) = _SIZES[t]
        box = [rng.uniform(-extent, extent), rng.uniform(-extent, extent), rng.uniform(-1, 2), rng.uniform(l0, l1),
               rng.uniform(w0, w1), rng.uniform(h0, h1), rng.uniform(-math.pi, math.pi)]
        u = rng.random()
        level, points = (2, 30) if u < 0.1 else (0, 0) if u < 0.2 else (0, 3) if u < 0.35 else (int(rng.integers(0, 2)), 40)
        gts.append(make_object(f32(box), t, 1.0, ctx, ts, False, level, points))
    for _ in range(n_pd):
        if gts and rng.random() < 0.8:
            g = gts[int(rng.integers(len(gts)))]
            box, t = box_of(g), g['type']
            s = float(rng.choice([0.01, 0.03, 0.08, 0.2]))
            box[0] += rng.normal(0, s) * box[3]
            box[1] += rng.normal(0, s) * box[4]
            box[2] += rng.normal(0, s) * 0.5
            for k in (3, 4, 5):
                box[k] *= 1 + rng.normal(0, s / 2)
            box[6] += rng.normal(0, s / 2) + (math.pi if rng.random() < 0.1 else 0.0)
        else:
            t = int(rng.choice(types))
            (l0, l1), (w0, w1), (h0, h1) = _SIZES[t]
            box = [rng.uniform(-extent, extent), rng.uniform(-extent, extent), rng.uniform(-1, 2), rng.uniform(l0, l1),
                   rng.uniform(w0, w1), rng.uniform(h0, h1), rng.uniform(-math.pi, math.pi)]
        preds.append(make_object(f32(box), t, rng.uniform(0.02, 1.0), ctx, ts, rng.random() < 0.05))
    return preds, gts


def frame_is_decisive(preds, gts, margin=1e-4):
    """False when float32 against float64 could flip a decision: a same-type pair's IoU within ``margin`` of its threshold,
    a prediction's two best candidates closer than ``margin``, or two equal scores among same-type predictions"""
    for t in THRESH:
        ps = [p for p in preds if p['type'] == t]
        gs = [g for g in gts if g['type'] == t]
        scores = [p['score'] for p in ps]
        if len(set(scores)) != len(scores):
            return False
        for p in ps:
            vals = sorted((iou3d(box_of(p), box_of(g)) for g in gs), reverse=True)
            if any(abs(v - THRESH[t]) < margin for v in vals):
                return False
            if len(vals) >= 2 and vals[0] > 0 and vals[0] - vals[1] < margin:
                return False
    return True


def decisive_frames(rng, sizes, ctx='seg', ts0=0, **kw):
    """frames of the given (n_pd, n_gt) sizes, each redrawn until decisive -> (preds, gts, drawn, redrawn)"""
    preds, gts, drawn, redrawn = [], [], 0, 0
    for f, (n_pd, n_gt) in enumerate(sizes):
        while True:
            p, g = random_frame(rng, n_pd, n_gt, ctx, ts0 + f, **kw)
            drawn += 1
            if frame_is_decisive(p, g):
                break
            redrawn += 1
        preds += p
        gts += g
    return preds, gts, drawn, redrawn
