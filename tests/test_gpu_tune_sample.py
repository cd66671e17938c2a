"""GPU suite: csrc/tune_sample.hip (ococc_tune_sample_count / _fill behind occ_ops.tune_sample, over the bytes of
ococc_occ_frame_mark) against the plain restatement of tests/tune_sample_ref.py: counts, xyz, labels, index and weights
bit for bit.  Grids of 1, 250, 1024 (one full 1024-cell pass), 1025 (a one-cell second pass), 2500 and 27 000 cells (the
tie case: two free cells of equal key on either side of the draw); 1, 64 and 65 RoIs; a RoI that is not kept, one whose
points all miss the grid, one without a free cell, npos == nneg, npos == nneg + 1, npos == 3 nneg + 2, three free cells
under 1021 observed ones; caps equal to a RoI's rows, one less, 1, and one that cuts lists longer than a pass."""
import numpy as np
import pytest
import torch

import tune_sample_ref as ref

pytestmark = pytest.mark.gpu


def _args(c, dev, keep=True):
    T = lambda a: torch.from_numpy(a).to(dev)
    return (T(c.sizes), T(c.dims), T(c.start), c.total, ref.V, T(c.local_xyz), T(c.pts_roi), T(c.row_seeds),
            T(c.row_keep) if keep else None)


def _assert_equal(got, exp):
    xyz, labels, index, weights, counts = got
    assert counts == exp[4]
    S = sum(counts)
    assert xyz.dtype == torch.float32 and tuple(xyz.shape) == (S, 3)
    assert labels.dtype == torch.int32 and index.dtype == torch.int32 and weights.dtype == torch.float32
    for g, e in zip((xyz, labels, index, weights), exp[:4]):
        assert g.cpu().numpy().tobytes() == e.tobytes()


SCENES = {
    'one-cell': lambda: ref.single_scene('one_cell_hit'),
    'one-full-tile': lambda: ref.single_scene('full_tile_even'),
    'mixed-64': lambda: ref.mixed_scene(64),
    'mixed-65': lambda: ref.mixed_scene(65, scene=1),
    'tie': ref.tie_scene,
}


@pytest.fixture(scope='module', params=list(SCENES), ids=list(SCENES))
def scene(request):
    return SCENES[request.param]()


def test_kernels_equal_the_restatement(scene, dev):
    from objectcentricocccompletion_amd.occ import occ_ops
    assert occ_ops.TUNE_SAMPLE_KERNEL
    c = scene
    for cap in ref.CAPS:
        exp = ref.run_case(c, True, cap)
        got = occ_ops.tune_sample(*_args(c, dev), balance=True, cap=cap)
        _assert_equal(got, exp)
        again = occ_ops.tune_sample(*_args(c, dev), balance=True, cap=cap)                  # two runs, equal bytes
        assert all(torch.equal(a, b) for a, b in zip(got[:4], again[:4])) and got[4] == again[4]
        index = got[2].cpu().numpy()
        assert (np.diff(index) >= 0).all()
    _assert_equal(occ_ops.tune_sample(*_args(c, dev), balance=False), ref.run_case(c, False, -1))
    _assert_equal(occ_ops.tune_sample(*_args(c, dev, keep=False), balance=True, cap=73), ref.run_case(c, True, 73, keep=False))


def test_the_cases_are_what_they_claim(dev):
    from objectcentricocccompletion_amd.occ import occ_ops
    c = ref.mixed_scene(65, scene=1)
    counts = dict(zip(c.kinds[:8], occ_ops.tune_sample(*_args(c, dev))[4][:8]))
    assert counts == dict(one_cell_hit=0, full_tile_even=1024, tile_plus_one=1026, sparse=74, not_kept=0, missed=1,
                          three_to_one=376, nearly_full=2042)
    t = ref.tie_scene()
    xyz, labels, index, _, counts = occ_ops.tune_sample(*_args(t, dev))
    ids = ref.cell_ids(t, xyz.cpu().numpy(), index.cpu().numpy())
    free = ids[labels.cpu().numpy() == 0]
    assert t.tie[0] in free and t.tie[1] not in free and counts == [2 * len(t.hits[0])]


def test_the_operator_chain_on_the_device_equals_the_kernels(dev, monkeypatch):
    from objectcentricocccompletion_amd.occ import occ_ops
    c = ref.mixed_scene(65, scene=1)
    for kw in (dict(balance=True, cap=-1), dict(balance=True, cap=73), dict(balance=False)):
        kernels = occ_ops.tune_sample(*_args(c, dev), **kw)
        monkeypatch.setattr(occ_ops, 'TUNE_SAMPLE_KERNEL', False)
        chain = occ_ops.tune_sample(*_args(c, dev), **kw)
        monkeypatch.setattr(occ_ops, 'TUNE_SAMPLE_KERNEL', True)
        assert kernels[4] == chain[4]
        assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(kernels[:4], chain[:4]))


def test_centres_are_those_of_dense_grid_cells(dev):
    from objectcentricocccompletion_amd.occ import occ_ops
    c = ref.mixed_scene(8)
    a = _args(c, dev)
    xyz, labels, index, _, counts = occ_ops.tune_sample(*a, balance=False)
    cells, box = occ_ops.dense_grid_cells(a[0], a[1], a[2], ref.V, 0, c.total, c.total)
    kept = torch.from_numpy(c.row_keep).to(dev).bool()[box.long()]
    assert torch.equal(xyz, cells[kept]) and torch.equal(index, box[kept])


def test_argument_refusals_are_errors(dev):
    """every refusal is an error code and a message: nothing here launches on bad arguments"""
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ import occ_ops
    c = ref.mixed_scene(8)
    sizes, dims, start, total, v, xyz, roi, seeds, keep = _args(c, dev)
    with pytest.raises(L.OcoccError, match='cap > 0 with balance == 0'):
        occ_ops.tune_sample(sizes, dims, start, total, v, xyz, roi, seeds, keep, balance=False, cap=8)
    with pytest.raises(L.OcoccError, match='row_seeds'):
        occ_ops.tune_sample(sizes, dims, start, total, v, xyz, roi, seeds.int(), keep)
    with pytest.raises(L.OcoccError, match='row_seeds'):
        occ_ops.tune_sample(sizes, dims, start, total, v, xyz, roi, seeds[:-1], keep)
    with pytest.raises(L.OcoccError, match='row_keep'):
        occ_ops.tune_sample(sizes, dims, start, total, v, xyz, roi, seeds, keep[:-1])
    with pytest.raises(L.OcoccError, match='start int64'):
        occ_ops.tune_sample(sizes, dims, start[:-1], total, v, xyz, roi, seeds, keep)
    with pytest.raises(L.OcoccError, match='local_xyz'):
        occ_ops.tune_sample(sizes, dims, start, total, v, xyz.double(), roi, seeds, keep)
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        occ_ops.tune_sample(sizes.cpu(), dims, start, total, v, xyz, roi, seeds, keep)
    # a total smaller than the table says: the count kernel reads no cell of the RoIs beyond it and reports them
    with pytest.raises(L.OcoccError, match='prefix table'):
        occ_ops.tune_sample(sizes, dims, start, total - 1, v, xyz, roi, seeds, keep)
    # the exports themselves
    buf = torch.zeros(64, dtype=torch.int64, device=dev)
    p = L.ptr(buf)
    assert L.lib.ococc_tune_sample_count(p, 8, p, 1, p, None, 0, 4, p, p, L.stream()) == -1
    assert b'cap > 0 with balance == 0' in L.lib.ococc_last_error()
    assert L.lib.ococc_tune_sample_count(p, -1, p, 1, p, None, 1, 4, p, p, L.stream()) == -1
    assert L.lib.ococc_tune_sample_count(p, 8, None, 1, p, None, 1, 4, p, p, L.stream()) == -1
    assert b'null pointer' in L.lib.ococc_last_error()
    assert L.lib.ococc_tune_sample_count(p, 8, p, 1, None, None, 1, 4, p, p, L.stream()) == -1
    assert L.lib.ococc_tune_sample_fill(p, 8, p, 1, p, p, 0.0, p, p, p, p, p, p, p, 4, L.stream()) == -1
    assert b'voxel_size' in L.lib.ococc_last_error()
    assert L.lib.ococc_tune_sample_fill(p, 8, p, 1, p, p, 0.2, p, p, p, None, p, p, p, 4, L.stream()) == -1
    assert L.lib.ococc_tune_sample_count(None, 0, None, 0, None, None, 1, 4, None, None, L.stream()) == 0   # K == 0: empty
    torch.cuda.synchronize()
