"""CPU suite of tests/voxel_ref.py, the float64 restatement that tests/test_gpu_voxel_edges.py holds the voxel scatter
kernels to: it agrees with torch.unique(dim=0) and with Tensor.scatter_reduce in float64, its arg with torch.argmax on
data without ties, its backward with autograd; the case table names the kernel each case takes; and the per-element
float32 bound is not tighter than float32 allows: a sequential float32 sum stays inside it in every case."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_ref as V        # noqa: E402

GRID_SAMPLE = ['rows-1', 'rows-65', 'runs-across-waves', 'dropped-run-then-key', 'all-negative', 'cells-1', 'cells-65537',
               'ndim3-one-at-1', 'ndim4-one-at-0']
SEGMENT_SAMPLE = ['boundary-387x97-shuffled', 'boundary-388x97-sorted', 'boundary-1x1', 'channels-65-run', 'rows-tail-65',
                  'all-dropped-elem', 'dropped-edges-run', 'gaps-elem', 'singles-shuffled-run', 'ints-run', 'zeros-elem',
                  'negative-singles-elem']


def _torch_unique(coors):
    keep = (coors >= 0).all(axis=1)
    inv = np.full((len(coors),), -1, np.int64)
    if not keep.any():
        return np.zeros((0, coors.shape[1]), np.int64), inv, np.zeros((0,), np.int64)
    rows, back, counts = torch.unique(torch.from_numpy(coors[keep]).long(), dim=0, return_inverse=True, return_counts=True)
    inv[keep] = back.numpy()
    return rows.numpy(), inv, counts.numpy()


@pytest.mark.parametrize('name', GRID_SAMPLE + ['big'])
def test_unique_rows_vs_torch(name):
    coors = V.big_grid_rows() if name == 'big' else V.GRID_CASES[name][1]
    rows, inv, counts = V.unique_rows(coors)
    trows, tinv, tcounts = _torch_unique(coors)
    assert rows.dtype == inv.dtype == counts.dtype == np.int32
    assert np.array_equal(rows, trows) and np.array_equal(inv, tinv) and np.array_equal(counts, tcounts)
    assert (inv >= 0).sum() == counts.sum()
    live = inv >= 0
    assert np.array_equal(rows[inv[live]], coors[live])
    if len(rows) > 1:       # lexicographic and strictly increasing
        d = np.diff(rows.astype(np.int64), axis=0)
        first = np.argmax(d != 0, axis=1)
        assert (d[np.arange(len(d)), first] > 0).all()


def test_unique_rows_takes_a_vector():
    rows, inv, counts = V.unique_rows(np.array([3, -1, 0, 3, 3]))
    assert rows.tolist() == [[0], [3]] and inv.tolist() == [1, -1, 0, 1, 1] and counts.tolist() == [1, 3]


def test_grid_cases_hold_what_they_claim():
    for name, (dims, coors) in V.GRID_CASES.items():
        assert coors.dtype == np.int32 and coors.shape[1] == len(dims)
        assert (coors < np.asarray(dims)).all(), name
    assert sorted(len(c) for d, c in V.GRID_CASES.values() if d == [5, 9])[:8] == [1, 63, 64, 65, 130, 255, 256, 257]
    _, c = V.GRID_CASES['runs-across-waves']
    assert (c[60:71] == c[60]).all() and (c[250:263] == c[250]).all() and (c[60] >= 0).all() and (c[250] >= 0).all()
    _, c = V.GRID_CASES['dropped-run-then-key']
    for row in (64, 131):
        assert (c[row - 5:row] < 0).any(axis=1).all() and (c[row] >= 0).all()
        assert ((c == c[row]).all(axis=1)).sum() == 1
    for cells, last in ((65536, 2047), (65537, 2048), (65569, 2049)):
        _, c = V.GRID_CASES[f'cells-{cells}']
        words = set((c[c >= 0] // 32).tolist())
        assert max(words) == last == (cells - 1) // 32 and {0, 1, 2047}.issubset(words)
        assert {0, 31, 32, cells - 1}.issubset(set(c.ravel().tolist()))
        if cells > 65536:
            assert 2048 in words
    assert V.scan_blocks(V.BIG_DIMS) == 4100 and V.scan_blocks(V.BIG_TWIN_DIMS) == 4095
    c = V.big_grid_rows().astype(np.int64)
    assert c.shape == (10000, 2) and (c < np.asarray(V.BIG_DIMS)).all()
    words = set(((c[:, 0] * V.BIG_DIMS[1] + c[:, 1])[(c >= 0).all(axis=1)] // 32).tolist())
    last = (V.BIG_DIMS[0] * V.BIG_DIMS[1] - 1) // 32
    assert {0, last, 2048 * 256 - 1, 2048 * 256, 2048 * 4096 - 1, 2048 * 4096}.issubset(words)
    above = c[:, 0] >= V.BIG_TWIN_DIMS[0]
    assert above.any() and (c[~above, 0] < V.BIG_TWIN_DIMS[0]).all()


def test_case_table_names_the_kernel():
    seen = set()
    for case in V.SEGMENT_CASES:
        assert (4 * case.segs > case.n) == (case.kernel == 'elem'), case.name
        assert V.takes_elem(case.n, case.segs) == (case.kernel == 'elem')
        feats, inv, go = V.segment_case_data(case)
        assert feats.shape == (case.n, case.c) and feats.dtype == np.float32
        assert inv.shape == (case.n,) and inv.dtype == np.int32 and inv.min() >= -1 and inv.max() < case.segs
        assert go.shape == (case.segs, case.c) and go.dtype == np.float32
        seen.add((case.kernel, case.values))
    assert seen == {(k, v) for k in ('elem', 'run') for v in ('normal', 'negative', 'ints', 'zeros')}
    for segs in (1, 16, 97):
        assert {(4 * segs - 1, segs), (4 * segs, segs)} <= {(k.n, k.segs) for k in V.SEGMENT_CASES}
    assert {k.c for k in V.SEGMENT_CASES} >= {1, 2, 3, 31, 32, 33, 63, 64, 65, 129}


def test_patterns_hold_what_they_claim():
    data = lambda name: V.segment_case_data(V.SEGMENT_CASE_BY_NAME[name])
    feats, inv, _ = data('dropped-edges-run')
    assert inv[0] == -1 and inv[-1] == -1
    live = np.flatnonzero(inv >= 0)
    heads = live[1:][np.diff(inv[live]) != 0]
    assert ((inv[heads - 1] == -1) | (inv[heads + 1] == -1) | (inv[heads - 2] == -1)).all()   # -1 at every boundary
    for name in ('gaps-run', 'gaps-elem'):
        _, inv, _ = data(name)
        counts = np.bincount(inv, minlength=9)
        assert counts[0] == 0 and counts[-1] == 0 and (counts[2:-1:2] == 0).all() and (counts[1::2] > 0).all()
    for name in ('singles-run', 'singles-shuffled-elem'):
        _, inv, _ = data(name)
        counts = np.bincount(inv)
        assert (counts[0::2] == 1).all() and (counts[1::2] >= 2).all()
    _, inv, _ = data('one-segment-of-three')
    assert (inv == 1).all() and len(inv) == 5000
    feats, _, _ = data('negative-run')
    assert (feats < 0).all()
    feats, inv, _ = data('ints-one-segment')
    assert set(np.unique(feats).tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    feats, _, _ = data('zeros-run')
    assert (np.signbit(feats) & (feats == 0)).any() and (~np.signbit(feats) & (feats == 0)).any()
    red = V.segment_reduce(feats, data('zeros-run')[1], 13, 'max')
    assert (red.out[red.counts > 0] == 0).all()


@pytest.mark.parametrize('name', SEGMENT_SAMPLE)
def test_segment_reduce_vs_torch_float64(name):
    case = V.SEGMENT_CASE_BY_NAME[name]
    feats, inv, go = V.segment_case_data(case)
    live = inv >= 0
    idx = torch.from_numpy(inv[live].astype(np.int64))[:, None].expand(-1, case.c)
    for mode, reduce in (('sum', 'sum'), ('mean', 'mean'), ('max', 'amax')):
        x = torch.from_numpy(feats[live]).double().requires_grad_(True)
        out = torch.zeros(case.segs, case.c, dtype=torch.float64).scatter_reduce(0, idx, x, reduce, include_self=False)
        red = V.segment_reduce(feats, inv, case.segs, mode)
        assert red.out.dtype == np.float64
        assert np.array_equal(red.counts, np.bincount(inv[live], minlength=case.segs))
        if mode == 'mean':
            assert np.allclose(red.out, out.detach().numpy(), rtol=1e-15, atol=0)
        elif mode == 'sum':
            assert np.allclose(red.out, out.detach().numpy(), rtol=0, atol=1e-15 * max(red.abs_sum.max(), 1) * case.n)
        else:
            assert np.array_equal(red.out, out.detach().numpy())
        grad = V.segment_reduce_bwd(go, inv, red.counts, red.arg, mode)
        assert grad.shape == feats.shape and (grad[~live] == 0).all()
        if mode != 'max' or case.values in ('normal', 'negative'):   # (amax's autograd splits a gradient among ties)
            out.backward(torch.from_numpy(go).double())
            assert np.allclose(grad[live], x.grad.numpy(), rtol=1e-15, atol=0)


@pytest.mark.parametrize('name', [k.name for k in V.SEGMENT_CASES if k.values in ('normal', 'negative')])
def test_arg_vs_torch_argmax(name):
    case = V.SEGMENT_CASE_BY_NAME[name]
    feats, inv, _ = V.segment_case_data(case)
    red = V.segment_reduce(feats, inv, case.segs, 'max')
    x = torch.from_numpy(feats).double()
    for seg in range(case.segs):
        rows = np.flatnonzero(inv == seg)
        if len(rows) == 0:
            assert (red.arg[seg] == -1).all() and (red.out[seg] == 0).all()
            continue
        assert len(np.unique(feats[rows], axis=0)) == len(rows)        # no ties to speak of
        assert np.array_equal(red.arg[seg], rows[torch.argmax(x[rows], dim=0).numpy()])


def test_arg_is_the_smallest_row_among_ties():
    feats = np.array([[1.0], [3.0], [-0.0], [3.0], [0.0], [3.0], [-1.0]])
    inv = np.array([0, 0, 1, 0, 1, -1, 1])
    red = V.segment_reduce(feats, inv, 3, 'max')
    assert red.out[:, 0].tolist() == [3.0, 0.0, 0.0] and red.arg[:, 0].tolist() == [1, 2, -1]
    assert red.counts.tolist() == [3, 3, 0] and red.abs_sum[:, 0].tolist() == [7.0, 1.0, 0.0]
    grad = V.segment_reduce_bwd(np.array([[5.0], [7.0], [9.0]]), inv, red.counts, red.arg, 'max')
    assert grad[:, 0].tolist() == [0, 5.0, 7.0, 0, 0, 0, 0]
    grad = V.segment_reduce_bwd(np.array([[6.0], [9.0], [1.0]]), inv, red.counts, None, 'mean')
    assert grad[:, 0].tolist() == [2.0, 2.0, 3.0, 2.0, 3.0, 0, 3.0]


@pytest.mark.parametrize('name', [k.name for k in V.SEGMENT_CASES])
def test_sequential_float32_sum_is_inside_the_bound(name):
    """the bound the GPU tests apply is one float32 itself meets: rows added one after the other in float32"""
    case = V.SEGMENT_CASE_BY_NAME[name]
    feats, inv, _ = V.segment_case_data(case)
    live = inv >= 0
    for mode in ('sum', 'mean'):
        red = V.segment_reduce(feats, inv, case.segs, mode)
        out = np.zeros((case.segs, case.c), np.float32)
        np.add.at(out, inv[live], feats[live])                 # unbuffered: in row order, every step rounded to float32
        if mode == 'mean':
            out = out / np.maximum(red.counts, 1).astype(np.float32)[:, None]
        assert out.dtype == np.float32
        assert (np.abs(out.astype(np.float64) - red.out) <= V.float32_bound(red, mode)).all()
        small, exact = V.float32_small_segments(feats, inv, case.segs, mode)
        assert np.array_equal(out[small], exact[small])
        assert small.sum() == ((red.counts == 1) | (red.counts == 2)).sum()
