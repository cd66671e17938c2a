"""The emit launch of ococc_object_grid_geometry_f32 split into roles (csrc/grid_geometry.hip): row workgroups per
(grid, slice) write coordinates, tables, pairs and order records, point workgroups per (grid, part of the slices) write
inv, point counts, feature rows and means.  The cases here sit where that split can go wrong and the benchmark-like
batches of test_gpu_grid_geometry.py do not reach: cells shared by points from both ends of a grid's point segment,
grids with every cell occupied (no padding rows, words full of voxels), an empty and a one-point grid between full
ones, and two calls back to back.  References: the general path (voxelize_scatter_mean(static=True) +
get_indice_pairs), float64 means on the host, and the order built by the stand-alone ops.row_order."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _check_order(rec, hdr, table, rows):
    """a valid order: a permutation of the rows; masks and the entries at the two lowest neighbour offsets as in the
    table; classes 3+ / 2 / 1 / 0 neighbours in that sequence; the header the stand-alone counting pass builds."""
    from objectcentricocccompletion_amd.spconv import ops
    rec, hdr = rec.cpu().long(), hdr.cpu().tolist()
    tab = table.cpu().long()
    perm, smask = rec[:, 0], rec[:, 1] & 0xffffffff
    assert torch.equal(perm.sort().values, torch.arange(rows))
    tmask = torch.zeros(rows, dtype=torch.long)
    for k in range(27):
        tmask |= (tab[k] >= 0).long() << k
    assert torch.equal(smask, tmask[perm])
    nb = smask & ~(1 << 13)
    low1 = nb & -nb
    nb2 = nb & (nb - 1)
    low2 = nb2 & -nb2
    for col, low in ((2, low1), (3, low2)):
        want = torch.full((rows,), -1, dtype=torch.long)
        has = low != 0
        kk = torch.tensor([int(v).bit_length() - 1 for v in low.tolist()])
        want[has] = tab[kk[has], perm[has]]
        assert torch.equal(rec[:, col], want)
    pc = torch.tensor([bin(int(v)).count('1') for v in nb.tolist()])
    cls = 3 - pc.clamp(max=3)
    assert bool((cls[1:] >= cls[:-1]).all())
    rb2 = ops.RulebookTables(True, 27)
    _, hdr2 = ops.row_order(rb2, table, rows)
    assert hdr == hdr2.cpu().tolist()


def _geometry(xyz, bidx, feats, vs, rng, shape, B, slices, dtype=torch.bfloat16, order=None):
    """object_grid_geometry; order = None: no row order asked for, False / True: the one-call path / ORDER_SIDE_STREAM"""
    from objectcentricocccompletion_amd.spconv import ops
    from objectcentricocccompletion_amd.voxel import object_grid_geometry
    keep = ops.DEFAULT_PAIRS_PER_ROW, ops.ORDER_SIDE_STREAM
    try:
        if order is not None:
            ops.DEFAULT_PAIRS_PER_ROW, ops.ORDER_SIDE_STREAM = 1.8, order
        got = object_grid_geometry(xyz, bidx, feats, [vs] * 3, rng, shape, B, out_dtype=dtype, slices=slices)
    finally:
        ops.DEFAULT_PAIRS_PER_ROW, ops.ORDER_SIDE_STREAM = keep
    assert got is not None
    return got


def _general(xyz, bidx, feats, vs, rng, shape, B, dtype=torch.bfloat16):
    from objectcentricocccompletion_amd.spconv import ops
    from objectcentricocccompletion_amd.voxel import voxelize_scatter_mean
    rf, rc, rinv, rcnt, rmeta = voxelize_scatter_mean(xyz, bidx, feats, [vs] * 3, rng, shape, B, static=True, out_dtype=dtype)
    _, rpairs, rnum = ops.get_indice_pairs(rc, B, shape, 3, subm=True)
    return rf, rc, rinv, rcnt, rmeta, rpairs, rnum


def _assert_tables_equal(got, ref):
    gf, gc, ginv, gcnt, gmeta, gpairs, gnum = got
    rf, rc, rinv, rcnt, rmeta, rpairs, rnum = ref
    torch.cuda.synchronize()
    assert gmeta.tolist() == rmeta.tolist()
    assert torch.equal(gc, rc) and torch.equal(ginv, rinv) and torch.equal(gcnt, rcnt)
    assert torch.equal(gnum, rnum)
    rt, rmask, _ = rpairs._ococc.tables[(False, 'fwd')]
    gt, gmask, _ = gpairs._ococc.tables[(False, 'fwd')]
    assert torch.equal(gt, rt) and torch.equal(gmask, rmask)
    for k in range(27):
        c = int(rnum[k])
        assert torch.equal(gpairs[k, :, :c], rpairs[k, :, :c]), k


def _assert_order_valid(got):
    from objectcentricocccompletion_amd.spconv import ops
    rb = got[5]._ococc
    table, _, rows = rb.tables[(False, 'fwd')]
    assert len(rb.orders) == 1
    rec, hdr = ops.row_order(rb, table, rows)
    _check_order(rec, hdr, table, rows)


# ---- cells shared across the point order ------------------------------------------------------------------------------
def _shared_cell_points():
    """3 grids of 40^3 cells at 0.2 m, 600 points each; in every grid one cell holds 5 points, one 3 and one 2, their
    copies at the two ends and in the middle of the grid's point segment (a split of the points by index would hand them
    to different workgroups); the three cells lie in different thirds of the grid's rows."""
    g = torch.Generator().manual_seed(11)
    B, P, G, vs = 3, 600, 40, 0.2
    where = {5: [0, 150, 300, 450, 599], 3: [1, 299, 598], 2: [2, 597]}
    xyz = []
    for b in range(B):
        cells = torch.randperm(G * G * G, generator=g)[:P].clone()
        zs = [(3 + 13 * ((j + b) % 3)) for j in range(3)]             # z planes of the shared cells: one per third
        for j, n in enumerate((5, 3, 2)):
            cell = (zs[j] * G + int(torch.randint(0, G, (1,), generator=g))) * G + int(torch.randint(0, G, (1,), generator=g))
            cells[cells == cell] = (cell + 7) % (G * G * G)            # (nobody else in it)
            cells[where[n]] = cell
        x, y, z = cells % G, (cells // G) % G, cells // (G * G)
        centre = torch.stack([x, y, z], 1).float() * vs - 4.0 + vs / 2
        xyz.append(centre + (torch.rand(P, 3, generator=g) - 0.5) * 0.16)
    xyz = torch.cat(xyz)
    feats = torch.randn(B * P, 16, generator=g)
    bidx = torch.repeat_interleave(torch.arange(B, dtype=torch.int32), P)
    return xyz, feats, bidx


@pytest.fixture(scope='module')
def shared_cells(dev):
    xyz, feats, bidx = _shared_cell_points()
    xyz, feats, bidx = xyz.to(dev), feats.to(dev), bidx.to(dev)
    args = (xyz, bidx, feats, 0.2, [-4.0] * 3 + [4.0] * 3, [40] * 3, 3)
    ref = {dt: _general(*args, dtype=dt) for dt in (torch.float32, torch.bfloat16)}
    torch.cuda.synchronize()
    rinv, rcnt = ref[torch.float32][2].cpu().numpy(), ref[torch.float32][3].cpu().numpy()
    f64 = feats.cpu().numpy().astype(np.float64)
    many = np.nonzero(rcnt > 2)[0]
    mean64 = np.stack([f64[rinv == r].mean(0) for r in many])
    # n - 1 float additions and one division: n * 2^-23 * mean|x_i| per channel
    bound = np.stack([rcnt[r] * 2.0 ** -23 * np.abs(f64[rinv == r]).mean(0) for r in many])
    return args, ref, many, mean64, bound


@pytest.mark.parametrize('slices', [1, 4, 13, None])
def test_shared_cells_meet_in_one_point_workgroup(shared_cells, slices):
    args, ref, many, mean64, bound = shared_cells
    rcnt = ref[torch.float32][3]
    assert sorted(rcnt[rcnt > 1].tolist()) == [2, 2, 2, 3, 3, 3, 5, 5, 5] and len(many) == 6
    for dt in (torch.float32, torch.bfloat16):
        got = _geometry(*args, slices, dtype=dt)
        rf, rc, rinv, _, rmeta = ref[dt][:5]
        torch.cuda.synchronize()
        assert got[4].tolist() == rmeta.tolist()
        assert torch.equal(got[1], rc) and torch.equal(got[2], rinv) and torch.equal(got[3], rcnt)
        few = rcnt <= 2
        assert torch.equal(got[0][few], rf[few])
        if dt == torch.float32:
            err = np.abs(got[0][torch.as_tensor(many, device=rf.device)].cpu().numpy().astype(np.float64) - mean64)
            print('rows with n > 2: largest error / bound', float((err / bound).max()))
            assert (err <= bound).all()


# ---- every cell occupied ----------------------------------------------------------------------------------------------
def _full_grids(shape, vs, fill, seed):
    """one point at the centre of every cell of the grids with fill[b] == 'full', a single point for 'one', none for
    'empty'; points of a grid in shuffled order"""
    g = torch.Generator().manual_seed(seed)
    gz, gy, gx = shape
    cells = gz * gy * gx
    xyz, bidx = [], []
    for b, kind in enumerate(fill):
        ids = {'full': torch.randperm(cells, generator=g), 'one': torch.tensor([cells // 3]), 'empty': torch.zeros(0, dtype=torch.long)}[kind]
        x, y, z = ids % gx, (ids // gx) % gy, ids // (gx * gy)
        lo = torch.tensor([-gx * vs / 2, -gy * vs / 2, -gz * vs / 2])
        xyz.append((torch.stack([x, y, z], 1).float() + 0.5) * vs + lo)
        bidx.append(torch.full((len(ids),), b, dtype=torch.int32))
    xyz, bidx = torch.cat(xyz), torch.cat(bidx)
    feats = torch.randn(len(xyz), 16, generator=g)
    rng = [-gx * vs / 2, -gy * vs / 2, -gz * vs / 2, gx * vs / 2, gy * vs / 2, gz * vs / 2]
    return xyz, feats, bidx, rng


@pytest.mark.parametrize('shape,vs', [((16, 16, 16), 0.5), ((8, 40, 40), 0.25)])
@pytest.mark.parametrize('slices', [1, 4])
def test_every_cell_occupied(dev, shape, vs, slices):
    xyz, feats, bidx, rng = _full_grids(shape, vs, ['full'], seed=shape[0] + slices)
    args = (xyz.to(dev), bidx.to(dev), feats.to(dev), vs, rng, list(shape), 1)
    ref = _general(*args)
    n = xyz.shape[0]
    assert int(ref[4][0]) == n == shape[0] * shape[1] * shape[2]           # V = n: no padding rows
    assert int(ref[6][0]) == (shape[0] - 1) * (shape[1] - 1) * (shape[2] - 1)   # a corner offset: interior rows have all 26
    for order in (False, True):
        got = _geometry(*args, slices, order=order)
        _assert_tables_equal(got, ref)
        _assert_order_valid(got)


# ---- an empty grid, and a one-point grid, between two full ones ----------------------------------------------------------
@pytest.mark.parametrize('middle', ['empty', 'one'])
@pytest.mark.parametrize('slices', [1, 4])
def test_empty_and_one_point_grid_between_full_ones(dev, middle, slices):
    shape, vs = (16, 16, 16), 0.5
    xyz, feats, bidx, rng = _full_grids(shape, vs, ['full', middle, 'full'], seed=3)
    args = (xyz.to(dev), bidx.to(dev), feats.to(dev), vs, rng, list(shape), 3)
    ref = _general(*args)
    for order in (False, True):
        got = _geometry(*args, slices, order=order)
        _assert_tables_equal(got, ref)
        _assert_order_valid(got)


# ---- two calls back to back -----------------------------------------------------------------------------------------------
def test_two_calls_back_to_back(dev):
    """the second call on the same stream, workspace and order counters, with other points: what the first one left
    (counters, finaliser marks in the point codes, block masks) does no harm"""
    g = torch.Generator().manual_seed(5)
    B, vs, shape, rng = 3, 0.2, [40] * 3, [-4.0] * 3 + [4.0] * 3
    sets = []
    for per_grid in (900, 500):
        n = B * per_grid
        xyz = (torch.rand(n, 3, generator=g) * 2 - 1) * 4.0
        xyz[: n // 20] = xyz[n // 20: 2 * (n // 20)]                       # shared cells -> finaliser marks
        feats = torch.randn(n, 16, generator=g)
        bidx = torch.repeat_interleave(torch.arange(B, dtype=torch.int32), per_grid)
        sets.append((xyz.to(dev), bidx.to(dev), feats.to(dev), vs, rng, shape, B))
    ref = _general(*sets[1])
    for order in (False, True):
        _geometry(*sets[0], 4, order=order)
        got = _geometry(*sets[1], 4, order=order)
        _assert_tables_equal(got, ref)
        few = ref[3] <= 2
        assert torch.equal(got[0][few], ref[0][few])
        _assert_order_valid(got)
