"""grid_unique, segment_count, segment_reduce (forward and backward) and the fused voxelize + mean front end against the
float64 numpy restatement tests/voxel_ref.py, at the places where these kernels take another path: the choice between
the element kernel and the run-length kernel (4 * segs > n), lanes per row and the second trip of the channel loop, rows
per wave (floor, cap, tails), the plain-store shortcut for segments of one row, the unsigned half of the float max
atomic, ties and both zeros in MAX; wave and block boundaries of the run-head shortcut of the cell marking, bitmap word
and scan tile boundaries of the popcount prefix, and the three-launch scan.

MAX, the counts, the rows and every backward are exact.  SUM and MEAN forward: the per-element float32 bound of
voxel_ref.float32_bound, derived there; segments of one or two rows equal the float32 result exactly."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_ref as V        # noqa: E402

pytestmark = pytest.mark.gpu

CODE = {'sum': 0, 'mean': 1, 'max': 2}


@functools.lru_cache(maxsize=None)
def _expected(name, mode):
    """computed once per (case, mode) and shared: callers do not write into it"""
    case = V.SEGMENT_CASE_BY_NAME[name]
    feats, inv, go = V.segment_case_data(case)
    red = V.segment_reduce(feats, inv, case.segs, mode)
    grad = V.segment_reduce_bwd(go, inv, red.counts, red.arg, mode)
    return feats, inv, go, red, grad


def _check_forward(out, feats, inv, segs, mode, red):
    """out: float32 numpy [segs, c] of the kernel"""
    if mode == 'max':
        assert np.array_equal(out, red.out)                # exact; +0.0 == -0.0
        return
    err = np.abs(out.astype(np.float64) - red.out)
    bound = V.float32_bound(red, mode)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), f'{mode}: |out - ref| = {err[worst]:.3e} > {bound[worst]:.3e} at {worst}'
    small, exact = V.float32_small_segments(feats, inv, segs, mode)
    assert np.array_equal(out[small], exact[small])
    assert (out[red.counts == 0] == 0).all()


def _expected_grad32(go, inv, red, grad64, mode):
    """the gradient as float32 arithmetic gives it: copies for sum and max, one correctly rounded division for mean"""
    live = inv >= 0
    seg = np.where(live, inv, 0)
    if mode == 'mean':
        exp = go[seg] / np.maximum(red.counts, 1).astype(np.float32)[seg][:, None]
        exp = np.where(live[:, None], exp, np.float32(0))
        assert exp.dtype == np.float32
        assert np.array_equal(exp, grad64.astype(np.float32))   # rounding the float64 quotient is the same number
        return exp
    exp = grad64.astype(np.float32)
    assert np.array_equal(exp.astype(np.float64), grad64)       # copies of float32 numbers and zeros
    return exp


@pytest.mark.parametrize('mode', V.MODES)
@pytest.mark.parametrize('name', [k.name for k in V.SEGMENT_CASES])
def test_segment_reduce_fwd_bwd(dev, name, mode):
    from objectcentricocccompletion_amd.voxel import segment_reduce
    case = V.SEGMENT_CASE_BY_NAME[name]
    assert V.takes_elem(case.n, case.segs) == (case.kernel == 'elem')
    assert (4 * case.segs > case.n) == (case.kernel == 'elem')
    feats, inv, go, red, grad64 = _expected(name, mode)
    exp_grad = _expected_grad32(go, inv, red, grad64, mode)
    inv_d, go_d = torch.from_numpy(inv).to(dev), torch.from_numpy(go).to(dev)
    counts_d = torch.from_numpy(red.counts.astype(np.int32)).to(dev)
    for counts in (counts_d, None):
        ft = torch.from_numpy(feats).to(dev).requires_grad_(True)
        out = segment_reduce(ft, inv_d, case.segs, mode, counts)
        assert out.dtype == torch.float32 and tuple(out.shape) == (case.segs, case.c)
        if counts is None and mode != 'sum':
            # the wrapper counted the rows itself (ococc_segment_count_i32) and keeps the result for the backward
            counted = out.grad_fn.saved_tensors[1]
            assert counted.dtype == torch.int32 and np.array_equal(counted.cpu().numpy(), red.counts)
        _check_forward(out.detach().cpu().numpy(), feats, inv, case.segs, mode, red)
        out.backward(go_d)
        got = ft.grad.cpu().numpy()
        assert np.array_equal(got, exp_grad)
        assert (got[inv < 0] == 0).all()
        if mode == 'max':   # each go[seg, ch] of an occupied segment lands on exactly one row: the smallest at the maximum
            hits = np.zeros((case.segs, case.c), np.int64)
            live = inv >= 0
            np.add.at(hits, inv[live], (red.arg[inv[live]] == np.flatnonzero(live)[:, None]).astype(np.int64))
            assert (hits[red.counts > 0] == 1).all() and (hits[red.counts == 0] == 0).all()


@pytest.mark.parametrize('mode', ['sum', 'max'])
@pytest.mark.parametrize('name', [k.name for k in V.SEGMENT_CASES])
def test_segment_reduce_without_counts_c_abi(dev, name, mode):
    """counts == NULL straight through the C ABI, as the backward of gather_rows calls it: no plain-store shortcut, no
    finalize pass -- empty segments are 0 for SUM and stay -inf for MAX; arg is the smallest row at the maximum"""
    from objectcentricocccompletion_amd import _lib as L
    case = V.SEGMENT_CASE_BY_NAME[name]
    assert (4 * case.segs > case.n) == (case.kernel == 'elem')
    feats, inv, _, red, _ = _expected(name, mode)
    ft, inv_d = torch.from_numpy(feats).to(dev), torch.from_numpy(inv).to(dev)
    out = torch.full((case.segs, case.c), 7.0, dtype=torch.float32, device=dev)
    arg = torch.full((case.segs, case.c), -5, dtype=torch.int32, device=dev) if mode == 'max' else None
    L.check(L.lib.ococc_segment_reduce_f32(L.ptr(ft), L.ptr(inv_d), case.n, case.c, CODE[mode], None, L.ptr(out),
                                           L.ptr(arg), case.segs, L.stream()), 'segment_reduce')
    counts = torch.full((case.segs,), -3, dtype=torch.int32, device=dev)
    L.check(L.lib.ococc_segment_count_i32(L.ptr(inv_d), case.n, L.ptr(counts), case.segs, L.stream()), 'segment_count')
    assert np.array_equal(counts.cpu().numpy(), red.counts)
    got = out.cpu().numpy()
    empty = red.counts == 0
    if mode == 'max':
        assert np.array_equal(got[~empty], red.out[~empty])
        assert (got[empty] == -np.inf).all()
        assert np.array_equal(arg.cpu().numpy()[~empty], red.arg[~empty])
    else:
        _check_forward(got, feats, inv, case.segs, mode, red)


# ------------------------------------------------------------------------------------------------------ grid_unique
def _grid_unique_equals_ref(dev, dims, coors):
    from objectcentricocccompletion_amd.voxel.scatter_points import grid_unique
    rows, inv, counts = V.unique_rows(coors)
    outc, ginv, gcounts = grid_unique(torch.from_numpy(coors).to(dev), dims=dims)
    assert outc.dtype == torch.int32 and ginv.dtype == torch.int32 and gcounts.dtype == torch.int32
    assert np.array_equal(outc.cpu().numpy().reshape(-1, rows.shape[1]), rows)
    assert np.array_equal(ginv.cpu().numpy(), inv)
    assert np.array_equal(gcounts.cpu().numpy(), counts)
    return rows, inv, counts


@pytest.mark.parametrize('name', list(V.GRID_CASES))
def test_grid_unique(dev, name):
    from objectcentricocccompletion_amd.voxel.scatter_points import grid_unique
    dims, coors = V.GRID_CASES[name]
    rows, inv, counts = _grid_unique_equals_ref(dev, dims, coors)
    if name == 'all-negative':
        assert len(rows) == 0 and (inv == -1).all()
    # the fixed-capacity form: the same on the first meta[0] rows, -1 coordinates and zero counts behind them
    outc, sinv, scounts, meta = grid_unique(torch.from_numpy(coors).to(dev), dims=dims, static=True)
    cells = int(np.prod(dims))
    num, status = meta.tolist()
    assert num == len(rows) and status == 0
    assert outc.shape[0] == scounts.shape[0] == min(len(coors), cells)
    outc, scounts = outc.cpu().numpy().reshape(-1, rows.shape[1]), scounts.cpu().numpy()
    assert np.array_equal(outc[:num], rows) and (outc[num:] == -1).all()
    assert np.array_equal(scounts[:num], counts) and (scounts[num:] == 0).all()
    assert np.array_equal(sinv.cpu().numpy(), inv)


@pytest.mark.parametrize('name', ['rows-65', 'cells-33', 'ndim3-one-at-1'])
def test_grid_unique_coordinate_at_its_bound(dev, name):
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.voxel.scatter_points import grid_unique
    dims, coors = V.GRID_CASES[name]
    coors = coors.copy()
    row = int(np.flatnonzero((coors >= 0).all(axis=1))[-1])
    coors[row, -1] = dims[-1]
    with pytest.raises(L.OcoccError):
        grid_unique(torch.from_numpy(coors).to(dev), dims=dims)
    *_, meta = grid_unique(torch.from_numpy(coors).to(dev), dims=dims, static=True)
    assert int(meta[1]) == 1


def test_grid_unique_three_launch_scan(dev):
    """268 697 600 cells are 4100 scan blocks: the block sums get a launch of their own.  The twin grid, 4095 blocks,
    takes the two-launch path on the rows both grids hold, which are the smaller cells: the same ranks and counts."""
    from objectcentricocccompletion_amd.voxel.scatter_points import grid_unique
    assert V.scan_blocks(V.BIG_DIMS) == 4100 > V.SCAN_TWO_LAUNCH_BLOCKS >= V.scan_blocks(V.BIG_TWIN_DIMS)
    coors = V.big_grid_rows()
    assert coors.shape == (10000, 2)
    rows, inv, counts = _grid_unique_equals_ref(dev, V.BIG_DIMS, coors)
    both = coors[:, 0] < V.BIG_TWIN_DIMS[0]
    assert 0 < (~both).sum() < 20
    toutc, tinv, tcounts = grid_unique(torch.from_numpy(coors[both]).to(dev), dims=V.BIG_TWIN_DIMS)
    num = tcounts.shape[0]
    assert num == len(rows) - len(np.unique(inv[~both]))
    assert np.array_equal(tinv.cpu().numpy(), inv[both])
    assert np.array_equal(tcounts.cpu().numpy(), counts[:num])
    assert np.array_equal(toutc.cpu().numpy(), rows[:num])


# --------------------------------------------------------------------------------------------------- fused front end
def test_fused_front_end_vs_float64(dev):
    """voxelize_scatter_mean on an independent answer: cells from the oracle's dynamic_voxelize, rows and means from
    voxel_ref"""
    from objectcentricocccompletion_amd.voxel import voxelize_scatter_mean
    from oracle import oracle as O
    n, batch, c, dup = 777, 2, 7, 0.5
    voxel, rng_, grid_zyx = [0.2, 0.2, 0.2], [-4, -4, -4, 4, 4, 4], [40, 40, 40]
    rng = np.random.default_rng(777)
    xyz = ((rng.random((n, 3)) * 2 - 1) * 4.2).astype(np.float32)          # a few land outside: clamped
    k = int(n * dup)
    src = rng.integers(0, n - k, size=k)
    xyz[n - k:] = xyz[src] + ((rng.random((k, 3)) - 0.5) * 1e-3).astype(np.float32)
    bidx = np.sort(rng.integers(0, batch, size=n)).astype(np.int32)
    bidx[n - k:] = bidx[src]
    feats = rng.standard_normal((n, c)).astype(np.float32)
    coors = np.concatenate([bidx[:, None], O.dynamic_voxelize(xyz, voxel, rng_)], axis=1)
    rows, inv, counts = V.unique_rows(coors)
    assert (counts >= 3).sum() >= 5                                      # the float atomics have something to reorder
    red = V.segment_reduce(feats, inv, len(rows), 'mean')
    vf, vc, ginv, gcnt, meta = voxelize_scatter_mean(torch.from_numpy(xyz).to(dev), torch.from_numpy(bidx).to(dev),
                                                     torch.from_numpy(feats).to(dev), voxel, rng_, grid_zyx, batch)
    assert meta.tolist() == [len(rows), 0]
    assert np.array_equal(vc.cpu().numpy(), rows)
    assert np.array_equal(ginv.cpu().numpy(), inv) and np.array_equal(gcnt.cpu().numpy(), counts)
    _check_forward(vf.cpu().numpy(), feats, inv, len(rows), 'mean', red)
