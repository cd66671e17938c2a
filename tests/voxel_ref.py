"""Plain numpy restatement, in float64, of the voxel scatter primitives (sorted unique rows with inverse and counts;
segment sum / mean / max with its backward), the checker of tests/test_voxel_ref_cpu.py and
tests/test_gpu_voxel_edges.py, and the table of cases both files walk.  It shares nothing with the package, the compiled
oracle or the kernels: np.unique for the rows, np.add.at / np.maximum.at for the reductions.

Error bound of a float32 sum (SUM, MEAN): m float32 terms added in ANY order (the kernels add run partials with float
atomics, in arrival order) differ from the exact sum by at most (m - 1) u sum|x| to first order, u = 2^-24 the unit
roundoff; the tests allow m u sum|x| per element and nothing global.  The division of MEAN is one more correctly
rounded operation: the bound over the count, plus u |ref|.  Segments of one or two rows have no order: a + b commutes,
the float32 result is exact."""
from collections import namedtuple

import numpy as np

U32 = 2.0 ** -24        # unit roundoff of float32


# ---------------------------------------------------------------------------------------------------- unique rows
def unique_rows(coors):
    """coors [N] or [N, ndim] integers -> (rows [U, ndim] int32: the distinct rows without a negative entry in
    lexicographic order, inv [N] int32: the position of each row in them, -1 for a row with a negative entry,
    counts [U] int32)"""
    coors = np.asarray(coors).astype(np.int64)
    if coors.ndim == 1:
        coors = coors[:, None]
    keep = (coors >= 0).all(axis=1)
    inv = np.full((coors.shape[0],), -1, np.int32)
    if not keep.any():
        return np.zeros((0, coors.shape[1]), np.int32), inv, np.zeros((0,), np.int32)
    rows, back, counts = np.unique(coors[keep], axis=0, return_inverse=True, return_counts=True)
    inv[keep] = np.asarray(back).reshape(-1)
    return rows.astype(np.int32), inv, counts.astype(np.int32)


# ------------------------------------------------------------------------------------------------ segment reduce
Reduced = namedtuple('Reduced', 'out counts arg abs_sum')


def segment_reduce(feats, inv, segs, mode):
    """feats [N, C], inv [N] in [-1, segs) -> Reduced(out [segs, C] float64, counts [segs] int64, arg [segs, C] int64
    (max only, else None): the smallest row index that attains the maximum, -1 for an empty segment,
    abs_sum [segs, C] float64 = sum |x|).  Empty segments give 0."""
    assert mode in ('sum', 'mean', 'max')
    x = np.asarray(feats).astype(np.float64)
    inv = np.asarray(inv).astype(np.int64)
    n, c = x.shape
    live = inv >= 0
    rows, seg = np.arange(n)[live], inv[live]
    counts = np.bincount(seg, minlength=segs).astype(np.int64)
    abs_sum = np.zeros((segs, c))
    np.add.at(abs_sum, seg, np.abs(x[live]))
    arg = None
    if mode == 'max':
        out = np.full((segs, c), -np.inf)
        np.maximum.at(out, seg, x[live])
        arg = np.full((segs, c), n, np.int64)
        at_max = x[live] == out[seg]                                # +0.0 == -0.0: either zero attains a zero maximum
        np.minimum.at(arg, seg, np.where(at_max, rows[:, None], n))
        out[counts == 0] = 0.0
        arg[counts == 0] = -1
    else:
        out = np.zeros((segs, c))
        np.add.at(out, seg, x[live])
        if mode == 'mean':
            out = out / np.maximum(counts, 1)[:, None]
    return Reduced(out, counts, arg, abs_sum)


def segment_reduce_bwd(go, inv, counts, arg, mode):
    """go [segs, C] -> the gradient [N, C] float64 of segment_reduce with respect to feats: sum copies go[inv], mean
    divides it by the count, max hands go[seg, ch] to row arg[seg, ch] alone; rows with inv = -1 get 0"""
    go = np.asarray(go).astype(np.float64)
    inv = np.asarray(inv).astype(np.int64)
    live = inv >= 0
    seg = np.where(live, inv, 0)
    g = go[seg]
    if mode == 'mean':
        g = g / np.maximum(np.asarray(counts), 1)[seg][:, None]
    elif mode == 'max':
        g = np.where(np.asarray(arg)[seg] == np.arange(inv.shape[0])[:, None], g, 0.0)
    return np.where(live[:, None], g, 0.0)


def float32_bound(red, mode):
    """per element: how far a float32 sum (mean) in any order may lie from red.out (module docstring)"""
    b = red.counts[:, None] * U32 * red.abs_sum
    if mode == 'mean':
        b = b / np.maximum(red.counts, 1)[:, None] + U32 * np.abs(red.out)
    return b


def float32_small_segments(feats, inv, segs, mode):
    """-> (mask [segs] of the segments with one or two rows, their float32 sum (mean) [segs, C]: exact, no order)"""
    x = np.asarray(feats, dtype=np.float32)
    inv = np.asarray(inv).astype(np.int64)
    live = inv >= 0
    counts = np.bincount(inv[live], minlength=segs)
    out = np.zeros((segs, x.shape[1]), np.float32)
    np.add.at(out, inv[live], x[live])
    if mode == 'mean':
        out = out / np.maximum(counts, 1).astype(np.float32)[:, None]
    return (counts >= 1) & (counts <= 2), out


# ------------------------------------------------------------------------------------------- segment reduce cases
# kernel: which of the two forward kernels of ococc_segment_reduce_f32 the case takes: 'elem' (thread per element) when
# 4 * segs > n, else 'run' (run-length walk, a wave per block of rows).  takes_elem() is the arithmetic; the tests
# assert that the table agrees with it, so that an edited shape cannot move a case to the other kernel unnoticed.
Case = namedtuple('Case', 'name n segs c pattern values kernel')


def takes_elem(n, segs):
    return 4 * segs > n


def _segment_cases():
    t = []

    def add(name, n, segs, c, pattern, values, kernel):
        t.append(Case(name, n, segs, c, pattern, values, kernel))

    # kernel boundary
    for segs in (1, 16, 97):
        for pattern in ('sorted', 'shuffled'):
            add(f'boundary-{4 * segs - 1}x{segs}-{pattern}', 4 * segs - 1, segs, 3, pattern, 'normal', 'elem')
            add(f'boundary-{4 * segs}x{segs}-{pattern}', 4 * segs, segs, 3, pattern, 'normal', 'run')
    add('boundary-1x1', 1, 1, 3, 'sorted', 'normal', 'elem')
    add('boundary-5x5', 5, 5, 3, 'shuffled', 'normal', 'elem')
    # channels: lanes per row 1 .. 64, a second trip of the channel loop from 65
    for c in (1, 2, 3, 31, 32, 33, 63, 64, 65, 129):
        add(f'channels-{c}-run', 1031, 13, c, 'dropped_edges', 'normal', 'run')
    for c in (1, 33, 65):
        add(f'channels-{c}-elem', 211, 60, c, 'shuffled', 'normal', 'elem')
    # rows per wave: the cap of 64 (c = 1, more than 8192 rows), tails at 32 rows per wave (c = 2), the floor of 4
    add('rows-cap', 8193, 64, 1, 'sorted', 'normal', 'run')
    for n in (64, 65, 127, 4097):
        add(f'rows-tail-{n}', n, 7, 2, 'sorted', 'normal', 'run')
    for n in (201, 1001):
        add(f'rows-floor-{n}', n, 5, 64, 'sorted', 'normal', 'run')
    # inv patterns
    add('one-segment', 5000, 1, 64, 'one', 'normal', 'run')
    add('one-segment-of-three', 5000, 3, 64, 'one', 'normal', 'run')
    add('all-dropped-run', 100, 5, 3, 'dropped_all', 'normal', 'run')
    add('all-dropped-elem', 10, 5, 3, 'dropped_all', 'normal', 'elem')
    add('dropped-edges-run', 517, 11, 5, 'dropped_edges', 'normal', 'run')
    add('dropped-edges-elem', 40, 11, 5, 'dropped_edges', 'normal', 'elem')
    add('gaps-run', 300, 9, 5, 'gaps', 'normal', 'run')
    add('gaps-shuffled-run', 300, 9, 5, 'gaps_shuffled', 'normal', 'run')
    add('gaps-elem', 30, 9, 5, 'gaps_shuffled', 'normal', 'elem')
    add('singles-run', 200, 30, 5, 'singles', 'normal', 'run')
    add('singles-shuffled-run', 200, 30, 5, 'singles_shuffled', 'normal', 'run')
    add('singles-elem', 41, 20, 5, 'singles', 'normal', 'elem')
    add('singles-shuffled-elem', 41, 20, 5, 'singles_shuffled', 'normal', 'elem')
    # values: all negative, integers (ties are the rule), both zeros
    for values in ('negative', 'ints', 'zeros'):
        add(f'{values}-run', 1031, 13, 5, 'dropped_edges', values, 'run')
        add(f'{values}-elem', 300, 100, 5, 'shuffled', values, 'elem')
        add(f'{values}-one-segment', 5000, 1, 64, 'one', values, 'run')
        add(f'{values}-singles-run', 200, 30, 5, 'singles_shuffled', values, 'run')
        add(f'{values}-singles-elem', 41, 20, 5, 'singles_shuffled', values, 'elem')
    return t


SEGMENT_CASES = _segment_cases()
SEGMENT_CASE_BY_NAME = {k.name: k for k in SEGMENT_CASES}
assert len(SEGMENT_CASE_BY_NAME) == len(SEGMENT_CASES)
MODES = ('sum', 'mean', 'max')


def _inv(pattern, n, segs, rng):
    if pattern in ('sorted', 'shuffled', 'dropped_edges'):
        inv = rng.integers(0, segs, size=n)
        if pattern != 'shuffled':
            inv = np.sort(inv)
        if pattern == 'dropped_edges':     # -1 on either side of run boundaries, at row 0 and at row n - 1
            heads = np.flatnonzero(np.diff(inv)) + 1
            inv[heads[::2]] = -1
            inv[heads[1::2] - 1] = -1
            inv[0] = inv[n - 1] = -1
        return inv
    if pattern == 'one':                   # one segment owns every row (the middle one: the others stay empty)
        return np.full((n,), segs // 2)
    if pattern == 'dropped_all':
        return np.full((n,), -1)
    if pattern in ('gaps', 'gaps_shuffled'):   # empty segments first, last and between occupied ones
        inv = rng.choice(np.arange(1, segs - 1, 2), size=n)
        return np.sort(inv) if pattern == 'gaps' else inv
    if pattern in ('singles', 'singles_shuffled'):   # even segments hold exactly one row, odd ones share the rest
        sizes = np.ones((segs,), np.int64)
        odd = np.arange(1, segs, 2)
        rest = n - (segs - len(odd))
        sizes[odd] = rest // len(odd)
        sizes[odd[-1]] += rest - sizes[odd].sum()
        assert sizes.sum() == n and (sizes[odd] >= 2).all()
        inv = np.repeat(np.arange(segs), sizes)
        return inv if pattern == 'singles' else inv[rng.permutation(n)]
    raise KeyError(pattern)


def _values(values, n, c, rng):
    if values == 'normal':
        return rng.standard_normal((n, c))
    if values == 'negative':
        return -(np.abs(rng.standard_normal((n, c))) + 0.25)
    if values == 'ints':
        return rng.integers(-2, 3, size=(n, c)).astype(np.float64)
    if values == 'zeros':                  # maxima are zeros of either sign, or -1 where a segment holds nothing else
        return rng.choice(np.array([0.0, -0.0, -1.0]), size=(n, c))
    raise KeyError(values)


def segment_case_data(case):
    """-> (feats [n, c] float32, inv [n] int32, go [segs, c] float32) of a case: the same arrays on every call"""
    rng = np.random.default_rng(1000 + SEGMENT_CASES.index(case))
    inv = _inv(case.pattern, case.n, case.segs, rng).astype(np.int32)
    feats = _values(case.values, case.n, case.c, rng).astype(np.float32)
    go = rng.standard_normal((case.segs, case.c)).astype(np.float32)
    return feats, inv, go


# --------------------------------------------------------------------------------------------- grid_unique cases
# name -> (dims, coors [n, ndim] int32): bounded coordinates; a row with a negative entry is dropped
def _grid_cases():
    t = {}
    rng = np.random.default_rng(77)

    def rand(n, dims, drop=0.1):
        c = np.stack([rng.integers(0, d, size=n) for d in dims], axis=1)
        c[rng.random(n) < drop, rng.integers(0, len(dims))] = -1
        return c

    # row counts around the wave (64) and the block (256)
    for n in (1, 63, 64, 65, 255, 256, 257, 513):
        t[f'rows-{n}'] = ([5, 9], rand(n, [5, 9]))
    c = rand(513, [5, 9])
    c[60:71] = [2, 3]                      # one key across the wave boundary at row 64,
    c[250:263] = [4, 8]                    # another across the block boundary at row 256
    t['runs-across-waves'] = ([5, 9], c)
    c = rand(257, [5, 9], drop=0.0)
    c[c[:, 0] == 4, 0] = 3                 # keys [4, *] are kept for the two rows below
    c[50:64] = -1
    c[64] = [4, 1]                         # a live key in lane 0, behind dropped rows
    c[120:131] = [2, -1]
    c[131] = [4, 2]                        # and in the middle of a wave
    t['dropped-run-then-key'] = ([5, 9], c)
    c = np.zeros((513, 2), np.int64)
    c[0::2], c[1::2] = [1, 7], [3, 0]
    t['two-keys-alternate'] = ([5, 9], c)
    t['all-rows-equal'] = ([5, 9], np.tile([[4, 8]], (513, 1)))
    t['all-negative'] = ([5, 9], np.tile([[2, -1]], (130, 1)))
    # 1-D cell counts: the last bitmap word is scan word 2047, 2048, 2049 for the last three
    for cells in (1, 31, 32, 33, 65536, 65537, 65569):
        # cell 0 and cells - 1; bit 31 and bit 0 of the next word; words 2047 and 2048 together
        marks = [0, cells - 1, 31, 32, 63, 64, 2047 * 32, 2047 * 32 + 31, 2048 * 32, 2048 * 32 + 31, 2049 * 32]
        marks = [m for m in marks if 0 <= m < cells]
        c = np.concatenate([np.repeat(marks, 2), rng.integers(0, cells, size=300), [-1] * 5])
        t[f'cells-{cells}'] = ([cells], rng.permutation(c)[:, None])
    # a dimension of size 1 in every position
    for ndim in (2, 3, 4):
        for pos in range(ndim):
            dims = [5, 7, 3, 6][:ndim]
            dims[pos] = 1
            t[f'ndim{ndim}-one-at-{pos}'] = (dims, rand(257, dims))
    return {k: (d, np.ascontiguousarray(c, dtype=np.int32)) for k, (d, c) in t.items()}


GRID_CASES = _grid_cases()

# the scan of the bitmap words takes a third launch above 4096 blocks of 2048 words
SCAN_TILE, SCAN_TWO_LAUNCH_BLOCKS = 2048, 4096


def scan_blocks(dims):
    cells = int(np.prod(np.asarray(dims, dtype=np.int64)))
    words = (cells + 31) // 32
    return (words + SCAN_TILE - 1) // SCAN_TILE


BIG_DIMS, BIG_TWIN_DIMS = [8200, 32768], [8190, 32768]


def big_grid_rows(n=10000):
    """rows for BIG_DIMS: cells in the first and the last bitmap word, on both sides of words 2048 * 256 and 2048 * 4096
    (where the block-sum scan starts its second trip, and where the two-launch scan would end), the rest at random
    below the twin's bound"""
    rng = np.random.default_rng(4100)
    width = BIG_DIMS[1]
    cells = [0, 5, 31, BIG_DIMS[0] * width - 1, BIG_DIMS[0] * width - 32]
    for word in (SCAN_TILE * 256, SCAN_TILE * SCAN_TWO_LAUNCH_BLOCKS):
        cells += [word * 32 - 32, word * 32 - 1, word * 32, word * 32 + 31]
    cells = np.asarray(cells, dtype=np.int64)
    special = np.stack([cells // width, cells % width], axis=1)
    special = np.concatenate([special, special[::2]])               # some of them twice
    rest = np.stack([rng.integers(0, BIG_TWIN_DIMS[0], size=n - len(special)),
                     rng.integers(0, width, size=n - len(special))], axis=1)
    rest[:200] = rest[200:400]                                      # repeated keys among the random ones
    rest[rng.integers(0, len(rest), size=50), 1] = -1
    return np.ascontiguousarray(rng.permutation(np.concatenate([special, rest])), dtype=np.int32)
