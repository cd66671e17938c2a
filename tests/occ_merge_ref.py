"""The occupancy-enhanced cloud of csrc/occ_merge.hip restated in plain numpy (boolean index, np.concatenate, np.pad),
and the cases tests/test_gpu_occ_merge.py runs.  No device, no package import."""
import numpy as np

F = np.float32
NAN_A = np.array([0x7fc12345], np.uint32).view(F)[0]      # two NaNs with payloads and a signalling one
NAN_B = np.array([0xffc00001], np.uint32).view(F)[0]
NAN_S = np.array([0x7f800001], np.uint32).view(F)[0]
DENORM = np.array([0x00000001], np.uint32).view(F)[0]     # the smallest positive denormal
DENORM_NEG = np.array([0x80000123], np.uint32).view(F)[0]


def use_dim_list(use_dim):
    return list(range(use_dim)) if isinstance(use_dim, int) else [int(v) for v in use_dim]


def occ_merge_ref(points, occ, counts, use_dim=(0, 1, 2, 3, 4), row_score=None, flags=None, drop_observed=False,
                  score_threshold=0.0):
    """(merged [N + K, D + 2] f32, survivors per row as a list): points [N, C] f32, occ [M, 4] f32, counts the cells
    per row.  A cell survives iff its score -- row_score[row], else its column 3 -- is > score_threshold in f32 and,
    with flags and drop_observed, bit 1 of its flag is clear."""
    points, occ = np.asarray(points, F), np.asarray(occ, F).reshape(-1, 4)
    dim = use_dim_list(use_dim)
    assert 3 <= len(dim) <= 16 and all(0 <= d < points.shape[1] for d in dim)
    counts = [int(c) for c in counts]
    assert sum(counts) == len(occ)
    row = np.repeat(np.arange(len(counts)), counts)
    score = np.asarray(row_score, F)[row] if row_score is not None else occ[:, 3]
    with np.errstate(invalid='ignore'):
        keep = score > F(score_threshold)
    if flags is not None and drop_observed:
        keep &= (np.asarray(flags, np.uint8) & 2) == 0
    head = np.pad(points[:, dim], ((0, 0), (0, 2)), mode='constant', constant_values=0)
    tail = np.pad(occ[keep][:, :3], ((0, 0), (0, len(dim) - 3)), mode='constant', constant_values=0)
    tail = np.concatenate([tail, score[keep][:, None]], axis=1)
    tail = np.pad(tail, ((0, 0), (0, 1)), mode='constant', constant_values=1)
    merged = np.concatenate([head, tail], axis=0).astype(F, copy=False)
    return merged, np.bincount(row[keep], minlength=len(counts)).tolist()


def _cloud(rng, n, c=6):
    pts = rng.normal(0, 20, (n, c)).astype(F)
    if n >= 3:                                   # payload that arithmetic would change
        pts[0, 0], pts[1, 3], pts[2, c - 1], pts[n // 2, 1] = NAN_A, DENORM, NAN_B, DENORM_NEG
    return pts


def _cells(rng, m, threshold):
    """cells whose column 3 lies around the threshold, about half above"""
    occ = rng.normal(0, 5, (m, 4)).astype(F)
    occ[:, 3] = (F(threshold) + rng.normal(0, 0.2, m)).astype(F) if np.isfinite(threshold) else rng.random(m).astype(F)
    if m >= 4:
        occ[0, 0], occ[1, 2], occ[m - 1, 1] = NAN_S, DENORM, NAN_A
    return occ


def case(name, n, counts, use_dim=(0, 1, 2, 3, 4), threshold=0.25, seed=0, row_score=None, flags=None, drop=False,
         occ=None, c=6):
    rng = np.random.default_rng(seed)
    m = int(sum(counts))
    occ = _cells(rng, m, threshold) if occ is None else np.asarray(occ, F)
    if isinstance(row_score, str):
        row_score = (F(threshold) + rng.normal(0, 0.2, len(counts))).astype(F)
    if isinstance(flags, str):
        flags = rng.integers(1, 4, m).astype(np.uint8)
    return dict(name=name, points=_cloud(rng, n, c), occ=occ, counts=list(counts), use_dim=use_dim,
                row_score=row_score, flags=flags, drop_observed=drop, score_threshold=threshold)


STRADDLE = [0, 1024, 5000, 0, 1500, 373, 0]      # empty rows first, in the middle and last; one tile exactly; two blocks of tiles


def edge_scores(threshold):
    t = F(threshold)
    return np.array([t, np.nextafter(t, F(np.inf)), np.nextafter(t, F(-np.inf)), np.nan, np.inf, -np.inf, -0.0, 0.0,
                     DENORM, DENORM_NEG, NAN_A], F)


def cases():
    out = []
    for m in (0, 1, 1023, 1024, 1025, 4096, 4097):
        out.append(case(f'M{m}', 65, [m], seed=m))
    out.append(case('R0', 64, []))
    out.append(case('R7', 65, STRADDLE, seed=7))
    out.append(case('R7_row_score', 65, STRADDLE, seed=8, row_score=np.array([0.9, 0.3, 0.1, 0.9, 0.4, 0.2, 0.9], F)))
    out.append(case('R7_short', 63, [0, 3, 0, 0, 2, 1, 0], seed=9))
    for n in (0, 1, 63, 64, 65, 1025, 3001):     # 3001 * 7 = 21007 elements: eleven copy blocks, the last one short
        out.append(case(f'N{n}', n, [40, 0, 33], seed=100 + n))
    out.append(case('N0_M0', 0, []))
    out.append(case('N0_M0_R2', 0, [0, 0]))
    for dim in ((0, 1, 2), (0, 1, 2, 3, 4), (0, 1, 2, 3, 4, 5), (2, 0, 1, 5), (0, 1, 2, 3, 3), 4):
        out.append(case(f'dim{dim}', 130, [700, 1100], use_dim=dim, seed=11))
    for thr in (0.25, 0.0):
        sc = edge_scores(thr)
        cells = np.random.default_rng(5).normal(0, 5, (len(sc), 4)).astype(F)
        cells[:, 3] = sc
        out.append(case(f'edges_col3_{thr}', 7, [len(sc)], threshold=thr, occ=cells))
        out.append(case(f'edges_col3_rows_{thr}', 7, [3, 0, len(sc) - 3], threshold=thr, occ=cells))
        out.append(case(f'edges_row_score_{thr}', 7, [2] * len(sc), threshold=thr, row_score=sc, seed=3))
    for drop in (False, True):
        out.append(case(f'flags_drop{int(drop)}', 65, STRADDLE, seed=21, flags='random', drop=drop))
        out.append(case(f'flags_row_score_drop{int(drop)}', 65, [5, 1030, 0], seed=22, flags='random', drop=drop,
                        row_score=np.array([0.9, 0.5, 0.1], F)))
    out.append(case('flags_all_observed', 5, [1500], seed=23, flags=np.full(1500, 2, np.uint8), drop=True))
    out.append(case('all_survive', 65, STRADDLE, threshold=-np.inf, seed=31))
    out.append(case('none_survive', 65, STRADDLE, threshold=np.inf, seed=32))
    return out
