"""The observation sample of a tuned online step restated in plain numpy, RoI by RoI: the integer mixer,
the selection rule, the cap and the weights.  This file is the definition the kernels of csrc/tune_sample.hip and the
operator chain occ_ops.tune_sample_aten are compared against, bit for bit; it shares no code with either."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
CAP_SALT = np.uint64(0xD1B54A32D192ED03)
M64 = (1 << 64) - 1


def mix64(x):
    """The splitmix64 finaliser on a uint64 array (wrapping arithmetic)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over='ignore'):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def mix64_int(x):
    """mix64 of one Python int."""
    x &= M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def key(row_seed, c):
    """key(row_seed, c) = high 32 bits of mix64(row_seed + (c + 1) * golden): uint64 array of values < 2^32."""
    c = np.asarray(c, dtype=np.uint64)
    with np.errstate(over='ignore'):
        x = np.uint64(int(row_seed) & M64) + (c + np.uint64(1)) * GOLDEN
    return mix64(x) >> np.uint64(32)


def cap_key(row_seed, p):
    return key((int(row_seed) & M64) ^ int(CAP_SALT), p)


def row_seed(seed, slot, frame):
    """The seed of the row of (slot, frame) under the call's ``seed``, as a signed 64-bit Python int."""
    v = mix64_int((int(seed) & M64) ^ (((int(slot) << 32) | int(frame)) & M64))
    return v - (1 << 64) if v >= (1 << 63) else v


def smallest(keys, idx, q):
    """The q members of ``idx`` with the smallest (key, index)."""
    order = np.lexsort((idx, keys))
    return idx[order[:q]]


def mark(sizes, dims, start, total, voxel_size, local_xyz, pts_roi):
    """observed [total] uint8: quantize_points' expression in f32 with a true division, as tests/occ_frame_ref.py."""
    seen = np.zeros(int(total), dtype=np.uint8)
    vs = np.float32(voxel_size)
    for p, r in zip(np.asarray(local_xyz, dtype=np.float32), np.asarray(pts_roi)):
        r = int(r)
        if r < 0 or r >= len(sizes):
            continue
        lo = -sizes[r].astype(np.float32) / np.float32(2.0)
        q = np.floor((p - lo) / vs)
        d = dims[r]
        if not np.all((q >= 0) & (q < d)):
            continue
        q = q.astype(np.int64)
        seen[int(start[r]) + (q[0] * d[1] + q[1]) * d[2] + q[2]] = 1
    return seen


def centres(size, dim, voxel_size):
    """dense_voxel_centers_batched's expression for one box: x slowest, z fastest, f32, operator by operator."""
    vs = np.float32(voxel_size)
    g = np.stack(np.meshgrid(np.arange(dim[0]), np.arange(dim[1]), np.arange(dim[2]), indexing='ij'), -1).reshape(-1, 3)
    at = g.astype(np.float32) * vs
    lo = at + (-size.astype(np.float32) / np.float32(2.0))[None, :]
    return (lo + vs / np.float32(2.0)).astype(np.float32)


def roi_rows(observed, seed, keep, balance, cap):
    """(cells, labels) of one RoI: ``observed`` its k bytes.  Cells in grid order, copies adjacent."""
    k = observed.size
    cells = np.zeros((0,), dtype=np.int64)
    if not keep or k == 0:
        return cells, cells
    obs = observed != 0
    if not balance:
        assert cap <= 0
        c = np.arange(k)
        return c, obs.astype(np.int64)
    npos = int(obs.sum())
    nneg = k - npos
    if npos == 0:
        return np.array([0]), np.array([0])
    if nneg == 0:
        return cells, cells
    free = np.nonzero(~obs)[0]
    mult = obs.astype(np.int64)
    fkeys = key(seed, free)
    if npos <= nneg:
        mult[smallest(fkeys, free, npos)] = 1
    else:
        mult[free] = npos // nneg
        mult[smallest(fkeys, free, npos % nneg)] += 1
    cells = np.repeat(np.arange(k), mult)
    if cap > 0 and cells.size > cap:
        pos = np.arange(cells.size)
        cells = cells[np.sort(smallest(cap_key(seed, pos), pos, cap))]
    return cells, obs[cells].astype(np.int64)


def tune_sample_ref(sizes, dims, start, total, voxel_size, local_xyz, pts_roi, row_seeds, row_keep, balance=True, cap=-1):
    """(xyz [S, 3] f32, labels [S] i32, index [S] i32, weights [S] f32, counts [K] list)."""
    sizes, dims, start = np.asarray(sizes, np.float32), np.asarray(dims), np.asarray(start)
    seen = mark(sizes, dims, start, total, voxel_size, local_xyz, pts_roi)
    xyz, lab, idx, wts, counts = [], [], [], [], []
    for r in range(len(sizes)):
        keep = True if row_keep is None else bool(row_keep[r])
        cells, labels = roi_rows(seen[int(start[r]):int(start[r + 1])], int(row_seeds[r]), keep, balance, cap)
        m = cells.size
        counts.append(m)
        if m == 0:
            continue
        xyz.append(centres(sizes[r], dims[r], voxel_size)[cells])
        lab.append(labels.astype(np.int32))
        idx.append(np.full(m, r, dtype=np.int32))
        wts.append(np.full(m, np.float32(1.0) / np.float32(m), dtype=np.float32))
    if not xyz:
        z = np.zeros((0,), np.int32)
        return np.zeros((0, 3), np.float32), z, z, np.zeros((0,), np.float32), counts
    return np.concatenate(xyz), np.concatenate(lab), np.concatenate(idx), np.concatenate(wts), counts


# ---------------------------------------------------------------------------------------------------------------------
# the inputs both test files run: built from dims and the cells to hit, so that every case is what it claims
V = 0.2
TIE_DIMS = (30, 30, 30)
# RoI kinds of the mixed scenes: (dims, observed cells as a function of the cell count, keep, points outside the grid)
KINDS = (
    ('one_cell_hit', (1, 1, 1), lambda k: 1, 1, 0),              # nneg == 0: no rows
    ('full_tile_even', (16, 8, 8), lambda k: k // 2, 1, 0),      # 1024 cells, npos == nneg
    ('tile_plus_one', (41, 5, 5), lambda k: k // 2 + 1, 1, 0),   # 1025 cells, npos == nneg + 1
    ('sparse', (25, 10, 10), lambda k: 37, 1, 3),                # 2500 cells, npos <= nneg, 74 rows
    ('not_kept', (25, 10, 10), lambda k: 20, 0, 0),              # keep == 0: no rows
    ('missed', (10, 5, 5), lambda k: 0, 1, 4),                   # npos == 0 with points present: cell 0, label 0
    ('three_to_one', (10, 5, 5), lambda k: 188, 1, 0),           # 250 cells, npos == 3 nneg + 2
    ('nearly_full', (16, 8, 8), lambda k: k - 3, 1, 0),          # 1024 cells, 3 free: 340 copies each, one 341
)
CAPS = (-1, 1, 73, 74, 600)   # 74 == m_r and 73 == m_r - 1 of 'sparse'; 600 cuts lists that pass a 1024-cell pass


class Case(object):
    pass


def _scene(dims_list, hit_lists, keep, outside, seeds):
    c = Case()
    c.dims = np.asarray(dims_list, dtype=np.int32).reshape(-1, 3)
    c.sizes = ((c.dims.astype(np.float64) - 0.5) * V).astype(np.float32)     # ceil(size / V) == dims
    cells = c.dims.astype(np.int64).prod(1)
    c.start = np.concatenate([[0], np.cumsum(cells)]).astype(np.int64)
    c.total = int(c.start[-1])
    pts, roi = [], []
    for r, hits in enumerate(hit_lists):
        ctr = centres(c.sizes[r], c.dims[r], V)
        pts.append(ctr[np.asarray(hits, dtype=np.int64)])
        far = np.tile(c.sizes[r] / 2 + np.float32(0.15), (outside[r], 1)).astype(np.float32)   # pooled from the enlarged box
        pts.append(far)
        roi += [r] * (len(hits) + outside[r])
    c.local_xyz = np.concatenate(pts).astype(np.float32).reshape(-1, 3)
    c.pts_roi = np.asarray(roi, dtype=np.int32)
    c.row_keep = np.asarray(keep, dtype=np.uint8)
    c.row_seeds = np.asarray(seeds, dtype=np.int64)
    c.hits = [np.asarray(h, dtype=np.int64) for h in hit_lists]
    return c


def mixed_scene(K, scene=0):
    """K RoIs cycling through KINDS, the observed cells of each drawn by numpy's generator."""
    rng = np.random.RandomState(100 + K)
    dims, hits, keep, outside, kinds = [], [], [], [], []
    for r in range(K):
        name, d, npos, kp, out = KINDS[r % len(KINDS)]
        k = d[0] * d[1] * d[2]
        dims.append(d), keep.append(kp), outside.append(out), kinds.append(name)
        hits.append(np.sort(rng.permutation(k)[:npos(k)]))
    c = _scene(dims, hits, keep, outside, [row_seed(0, r, scene) for r in range(K)])
    c.kinds = kinds
    return c


def single_scene(kind):
    name, d, npos, kp, out = [k for k in KINDS if k[0] == kind][0]
    k = d[0] * d[1] * d[2]
    c = _scene([d], [np.arange(k)[:npos(k)]], [kp], [out], [row_seed(0, 0, 7)])
    c.kinds = [name]
    return c


def find_tie():
    """(row seed, c1, c2): the first seed of row_seed(0, 0, frame) under which two cells c1 < c2 of a 27 000-cell RoI carry
    equal 32-bit keys (about one seed in twelve: 27000^2 / 2 / 2^32)."""
    k = TIE_DIMS[0] * TIE_DIMS[1] * TIE_DIMS[2]
    cells = np.arange(k)
    for frame in range(1000):
        s = row_seed(0, 0, frame)
        keys = key(s, cells)
        u, first, cnt = np.unique(keys, return_index=True, return_counts=True)
        if (cnt == 2).any() and not (cnt > 2).any():
            t = u[cnt == 2][0]
            c1, c2 = np.nonzero(keys == t)[0]
            return s, int(c1), int(c2)
    raise AssertionError('no tie in 1000 seeds')


def tie_scene():
    """One 27 000-cell RoI whose draw ends between two free cells of equal key: the observed cells are chosen so that the
    npos-th smallest free (key, cell) is (t, c1) -- c1 is drawn, c2 is not."""
    s, c1, c2 = find_tie()
    k = TIE_DIMS[0] * TIE_DIMS[1] * TIE_DIMS[2]
    cells = np.arange(k)
    keys = key(s, cells)
    below = np.nonzero((keys < keys[c1]))[0]                       # (key, c) < (t, c1)
    above = np.nonzero((keys > keys[c1]))[0]
    nb = below.size
    a = max(0, -(-(nb + 1 - above.size) // 2))
    b = nb + 1 - 2 * a
    assert 0 <= a <= nb and 0 <= b <= above.size
    hits = np.sort(np.concatenate([below[:a], above[:b]]))          # npos = a + b = (nb - a) + 1: the free ones below, and c1
    c = _scene([TIE_DIMS], [hits], [1], [0], [s])
    c.kinds, c.tie = ['tie'], (c1, c2)
    return c


def run_case(c, balance=True, cap=-1, keep=True):
    return tune_sample_ref(c.sizes, c.dims, c.start, c.total, V, c.local_xyz, c.pts_roi, c.row_seeds,
                           c.row_keep if keep else None, balance, cap)


def cell_ids(c, xyz, index):
    """the local cell id of every row, from its centre"""
    out = np.zeros(len(index), dtype=np.int64)
    for r in np.unique(index):
        sel = index == r
        lo = -c.sizes[r].astype(np.float64) / 2
        q = np.floor((xyz[sel].astype(np.float64) - lo) / V).astype(np.int64)
        d = c.dims[r].astype(np.int64)
        out[sel] = (q[:, 0] * d[1] + q[:, 1]) * d[2] + q[:, 2]
    return out
