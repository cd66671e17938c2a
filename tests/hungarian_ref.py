"""Plain Python restatement of rule 4b of the native Waymo detection metric (the Hungarian matcher per
score cutoff), the checker of tests/test_hungarian_ref_cpu.py and tests/test_gpu_waymo_hungarian.py.  It shares nothing
with csrc/frame_match.hip: rows carry their own potentials and partners, every prediction's private "stay unmatched"
column is a real entry of the candidate pool, and a step picks the minimum of that pool by an explicit key.

A group is the predictions of one (frame, type) in their packed order (descending score, file order) against the
ground-truth boxes in index order.  weights[i][j] is the integer weight of the edge (prediction i, ground truth j), 0
where there is no edge.  All arithmetic is integer."""
import math

import numpy as np

INF = 1 << 40


def weight(iou, threshold):
    """float32 IoU and threshold -> the edge's integer weight: (int)(iou * 1000.0f), the product in float32, for
    iou >= threshold; 0 (no edge) below it"""
    iou, threshold = np.float32(iou), np.float32(threshold)
    return int(np.float32(iou * np.float32(1000.0))) if iou >= threshold else 0


def weights_from_ious(ious, threshold):
    ious = np.asarray(ious, dtype=np.float32)
    return [[weight(v, threshold) for v in row] for row in ious]


def prefix_matchings(weights, n_cols=None):
    """Inserts the predictions one at a time, one shortest-augmenting-path search each (cost = -weight, integer
    potentials).  Yields after every insertion the matching of the predictions inserted so far: a list, per prediction
    the column it holds or -1.  The matching after n insertions has maximum total weight for the first n predictions.
    Ties in a search step: the smallest distance; at equal distance a ground-truth column before a private one, the
    lower index among ground-truth columns, the earlier-scanned row among private columns."""
    n = len(weights)
    m = (len(weights[0]) if n else 0) if n_cols is None else n_cols
    u, v = [0] * n, [0] * m
    row_on, col_of = [-1] * m, [-1] * n
    for cur in range(n):
        dist, came_from, closed = [INF] * m, [-1] * m, [False] * m
        private = []                    # (distance, scan order, row) of the private columns in the pool
        scanned = []
        i, reached = cur, 0
        while True:
            scanned.append(i)
            private.append((reached - u[i], len(private), i))      # cost 0, column potential 0
            for j in range(m):
                if not closed[j] and weights[i][j] > 0:
                    d = reached - weights[i][j] - u[i] - v[j]
                    if d < dist[j]:
                        dist[j], came_from[j] = d, i
            real = min(((dist[j], j) for j in range(m) if not closed[j] and dist[j] < INF), default=None)
            best_private = min(private)
            if real is not None and real[0] <= best_private[0]:
                reached, j = real
                closed[j] = True
                if row_on[j] < 0:
                    end = ('real', j)
                    break
                i = row_on[j]
            else:
                reached = best_private[0]
                end = ('private', best_private[2])
                break
        for i in scanned:
            u[i] += reached if i == cur else reached - dist[col_of[i]]
        for j in range(m):
            if closed[j]:
                v[j] -= reached - dist[j]
        if end[0] == 'real':
            j = end[1]
        elif end[1] == cur:
            j = -1
        else:                           # that row leaves its column for its private one
            j, col_of[end[1]] = col_of[end[1]], -1
            assert u[end[1]] == 0
        while j >= 0:
            i = came_from[j]
            row_on[j] = i
            j, col_of[i] = col_of[i], j
            if i == cur:
                break
        yield list(col_of[:cur + 1])


def total_weight(weights, matching):
    return sum(weights[i][j] for i, j in enumerate(matching) if j >= 0)


def cutoff_prefixes(scores):
    """scores of a group in its packed order (descending) -> per cutoff k = 0 .. 100 the number of predictions with
    score >= k / 100"""
    return [sum(1 for s in scores if s >= k / 100) for k in range(101)]


def cutoff_matchings(weights, scores, n_cols=None):
    """-> per cutoff k the matching of the predictions with score >= k / 100 (a list of columns or -1, one per such
    prediction)"""
    after = [[]] + list(prefix_matchings(weights, n_cols))
    return [after[n] for n in cutoff_prefixes(scores)]


# ------------------------------------------------------------------------------------------------ generated groups
def _box(x, y, l=4.0, w=2.0, h=1.5, yaw=0.0, z=0.5):
    return [float(np.float32(c)) for c in (x, y, z, l, w, h, yaw)]


def lattice_group(rng, n_pd, n_gt, step=0.5, cx=20.0, cy=-30.0):
    """equal axis-parallel boxes on a lattice: the IoU of a pair depends on the lattice offset only, so the weights take
    a handful of values and tie all the time; neighbouring ground-truth boxes overlap, so with a low threshold a
    prediction has many edges"""
    side = max(2, int(math.ceil(math.sqrt(max(n_pd, n_gt) * 1.3))))
    cells = [(a, b) for a in range(side) for b in range(side)]
    pick = lambda n: [cells[i] for i in rng.permutation(len(cells))[:n]]
    mk = lambda c: _box(cx + c[0] * step, cy + c[1] * step * 0.5)
    return [mk(c) for c in pick(n_pd)], [mk(c) for c in pick(n_gt)]


def cluster_group(rng, n_pd, n_gt, extent, cx=-40.0, cy=35.0):
    """random vehicle-like boxes with similar headings in a square of ``extent`` metres: dense and without structure
    for a small extent, sparse (most predictions without an edge) for a large one"""
    def mk():
        return _box(cx + rng.uniform(0, extent), cy + rng.uniform(0, extent), rng.uniform(3.5, 6.0), rng.uniform(1.6, 2.4),
                    rng.uniform(1.4, 2.2), rng.normal(0.3, 0.15), rng.uniform(0, 0.5))
    return [mk() for _ in range(n_pd)], [mk() for _ in range(n_gt)]


def duplicates_group(rng, n_pd, n_gt, cx=10.0, cy=60.0):
    """what real data looks like: ground truth that does not overlap, every prediction a perturbed copy of one box, so
    several predictions compete for one box at the shipped thresholds"""
    gts = [_box(cx + 8.0 * (k % 16), cy + 4.0 * (k // 16), rng.uniform(3.5, 6.0), rng.uniform(1.6, 2.4), rng.uniform(1.4, 2.2))
           for k in range(n_gt)]
    pds = []
    for _ in range(n_pd):
        if not gts:
            pds.append(_box(cx, cy))
            continue
        g = list(gts[int(rng.integers(len(gts)))])
        s = float(rng.choice([0.01, 0.03, 0.06]))
        g[0] += rng.normal(0, s) * g[3]
        g[1] += rng.normal(0, s) * g[4]
        g[6] += rng.normal(0, s)
        pds.append(_box(g[0], g[1], g[3], g[4], g[5], g[6], g[2]))
    return pds, gts


def generated_groups(seed=0):
    """-> list of (name, prediction boxes, ground-truth boxes, IoU threshold, scores).  Sizes 0 x n, n x 0, 1 x 1, ...,
    200 x 150; dense graphs (threshold 0.1) and sparse ones (the shipped thresholds); weights with many ties; scores
    from a coarse grid, so that cutoff buckets hold several predictions, in descending order."""
    rng = np.random.default_rng(seed)
    out = []

    def add(name, boxes, thr):
        pds, gts = boxes
        scores = np.sort(np.round(rng.uniform(0.0, 1.0, len(pds)) * rng.choice([10, 50, 200])) / rng.choice([10, 50, 200]))[::-1]
        scores = np.clip(scores, 0.0, 1.0)
        out.append((name, pds, gts, thr, [float(np.float32(s)) for s in scores]))

    add('0 x 5', lattice_group(rng, 0, 5), 0.1)
    add('6 x 0', lattice_group(rng, 6, 0), 0.1)
    add('1 x 1', lattice_group(rng, 1, 1), 0.1)
    for n_pd, n_gt in ((2, 3), (7, 4), (20, 20), (64, 65), (90, 40), (200, 150)):
        add(f'lattice {n_pd} x {n_gt}', lattice_group(rng, n_pd, n_gt), 0.1)
    add('lattice 40 x 30 at 0.5', lattice_group(rng, 40, 30), 0.5)
    for n_pd, n_gt in ((5, 5), (30, 45), (130, 70), (200, 150)):
        add(f'dense cluster {n_pd} x {n_gt}', cluster_group(rng, n_pd, n_gt, 3.0 + 0.05 * n_gt), 0.1)
    for n_pd, n_gt in ((12, 9), (80, 60), (200, 150)):
        add(f'sparse cluster {n_pd} x {n_gt}', cluster_group(rng, n_pd, n_gt, 60.0), 0.5)
    for n_pd, n_gt in ((9, 3), (80, 30), (200, 150)):
        add(f'duplicates {n_pd} x {n_gt}', duplicates_group(rng, n_pd, n_gt), 0.7)
    return out


HAND_1 = dict(weights=[[800, 750], [720, 0]], scores=[0.9, 0.8])     # A: g1 0.80, g2 0.75; B: g1 0.72
HAND_2 = dict(weights=[[720], [900]], scores=[0.9, 0.8])             # A: heading flipped, 0.72; B: 0.90
