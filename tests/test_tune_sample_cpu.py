"""The observation sample of a tuned online step without a GPU: the operator chain occ_ops.tune_sample_aten on CPU
tensors against the plain restatement of tests/tune_sample_ref.py on every case tests/test_gpu_tune_sample.py runs the
kernels on, the unbalanced form against OccAutoEncoder.sample_observation, the invariants of the balanced draw, its
uniformity over 512 seeds (bounds from the binomial distribution), the order of two cells of equal key, the argument
checks, and the declarations of the two exports."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import tune_sample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ('ococc_tune_sample_count', 'ococc_tune_sample_fill')


def _args(c, keep=True):
    T = torch.from_numpy
    return (T(c.sizes), T(c.dims), T(c.start), c.total, ref.V, T(c.local_xyz), T(c.pts_roi), T(c.row_seeds),
            T(c.row_keep) if keep else None)


def _aten(c, keep=True, **kw):
    from objectcentricocccompletion_amd.occ import occ_ops
    return occ_ops.tune_sample_aten(*_args(c, keep), **kw)


def _assert_equal(got, exp):
    xyz, labels, index, weights, counts = got
    assert counts == exp[4]
    assert xyz.dtype == torch.float32 and tuple(xyz.shape) == (sum(counts), 3)
    assert labels.dtype == torch.int32 and index.dtype == torch.int32 and weights.dtype == torch.float32
    for g, e in zip((xyz, labels, index, weights), exp[:4]):
        assert g.numpy().tobytes() == e.tobytes()


@pytest.fixture(scope='module')
def tie():
    return ref.tie_scene()


@pytest.fixture(scope='module')
def mixed():
    return ref.mixed_scene(65, scene=1)


@pytest.mark.parametrize('name', ['one-cell', 'one-full-tile', 'mixed-64', 'mixed-65', 'tie'])
def test_aten_chain_equals_the_restatement(name, tie, mixed):
    c = {'one-cell': lambda: ref.single_scene('one_cell_hit'), 'one-full-tile': lambda: ref.single_scene('full_tile_even'),
         'mixed-64': lambda: ref.mixed_scene(64), 'mixed-65': lambda: mixed, 'tie': lambda: tie}[name]()
    for cap in ref.CAPS:
        _assert_equal(_aten(c, balance=True, cap=cap), ref.run_case(c, True, cap))
    _assert_equal(_aten(c, balance=False), ref.run_case(c, False, -1))
    _assert_equal(_aten(c, keep=False, balance=True, cap=73), ref.run_case(c, True, 73, keep=False))


def test_the_cases_are_what_they_claim(mixed, tie):
    counts = dict(zip(mixed.kinds[:8], ref.run_case(mixed)[4][:8]))
    assert counts == dict(one_cell_hit=0, full_tile_even=1024, tile_plus_one=1026, sparse=74, not_kept=0, missed=1,
                          three_to_one=376, nearly_full=2042)
    cells = mixed.dims.astype(np.int64).prod(1)[:8].tolist()
    assert cells == [1, 1024, 1025, 2500, 2500, 250, 250, 1024] and int(np.prod(ref.TIE_DIMS)) == 27000
    seen = ref.mark(mixed.sizes, mixed.dims, mixed.start, mixed.total, ref.V, mixed.local_xyz, mixed.pts_roi)
    npos = [int(seen[mixed.start[r]:mixed.start[r + 1]].sum()) for r in range(8)]
    assert npos == [1, 512, 513, 37, 20, 0, 188, 1021] and 188 == 3 * (250 - 188) + 2
    assert (mixed.pts_roi == 5).sum() == 4                                     # 'missed' has points, none in its grid
    xyz, labels, index, weights, _ = ref.run_case(mixed)
    first = index == 5
    assert labels[first].tolist() == [0] and ref.cell_ids(mixed, xyz, index)[first].tolist() == [0]


def test_unbalanced_rows_are_sample_observation_of_the_kept_rois(mixed):
    """balance=False: rows, labels and index of OccAutoEncoder.sample_observation(downsample_size=-1,
    balance_sample=False) restricted to the kept RoIs, bit for bit"""
    from objectcentricocccompletion_amd.heads import OccAutoEncoder
    c = mixed
    K = len(c.dims)
    rois = torch.zeros(K, 8)
    rois[:, 0] = torch.arange(K)
    rois[:, 4:7] = torch.from_numpy(c.sizes)
    ae = types.SimpleNamespace(compensate_encoder_coors=True, voxel_size=ref.V, scale_wlh=[1.0, 1.0, 1.0],
                               offset_wlh=[0.0, 0.0, 0.0])
    centers, labels, box = OccAutoEncoder.sample_observation(ae, torch.from_numpy(c.local_xyz), rois,
                                                             torch.from_numpy(c.pts_roi), downsample_size=-1,
                                                             balance_sample=False)
    kept = torch.from_numpy(c.row_keep).bool()[box]
    xyz, lab, index, weights, counts = _aten(c, balance=False)
    assert xyz.numpy().tobytes() == centers[kept].numpy().tobytes()
    assert torch.equal(lab.long(), labels[kept]) and torch.equal(index.long(), box[kept])
    assert counts == (torch.bincount(box, minlength=K) * torch.from_numpy(c.row_keep).long()).tolist()


@pytest.mark.parametrize('cap', [-1, 1, 73, 600])
def test_balanced_invariants(mixed, cap):
    c = mixed
    xyz, labels, index, weights, counts = [a.numpy() if torch.is_tensor(a) else a for a in _aten(c, balance=True, cap=cap)]
    full = [a.numpy() if torch.is_tensor(a) else a for a in _aten(c, balance=True, cap=-1)]
    ids, full_ids = ref.cell_ids(c, xyz, index), ref.cell_ids(c, full[0], full[2])
    assert (np.diff(index) >= 0).all()
    for r in range(len(c.dims)):
        sel = index == r
        m = int(sel.sum())
        assert m == counts[r]
        k = int(c.start[r + 1] - c.start[r])
        npos, nneg = len(c.hits[r]), k - len(c.hits[r])
        kind = c.kinds[r]
        if kind in ('one_cell_hit', 'not_kept'):
            assert m == 0
            continue
        if kind == 'missed':
            assert m == 1
            continue
        f = full[2] == r
        pos_ids, neg_ids = full_ids[f][full[1][f] == 1], full_ids[f][full[1][f] == 0]
        assert np.array_equal(pos_ids, c.hits[r])                               # every observed cell exactly once, in order
        assert len(neg_ids) == npos and not np.isin(neg_ids, c.hits[r]).any()   # as many free rows as observed ones
        mult = np.bincount(neg_ids, minlength=k)
        if npos <= nneg:
            assert mult.max() == 1
        else:
            free = np.setdiff1d(np.arange(k), c.hits[r])
            assert mult[free].max() - mult[free].min() <= 1 and mult[free].min() == npos // nneg
        assert (np.diff(full_ids[f]) >= 0).all()                                # grid order, copies adjacent
        assert m == (min(cap, 2 * npos) if cap > 0 else 2 * npos)               # the cap is honoured
        # the capped rows are a sub-list of the uncapped ones, in list order
        it = iter(zip(full_ids[f].tolist(), full[1][f].tolist()))
        assert all(any(row == cand for cand in it) for row in zip(ids[sel].tolist(), labels[sel].tolist()))
        w = weights[sel]
        assert (w == w[0]).all() and abs(float(w[0]) * m - 1.0) <= 2.0 ** -23   # weights * m_r == 1 to one ulp
        assert w[0] == np.float32(1.0) / np.float32(m)


def _uniform_scene(n_seeds, npos):
    """n_seeds RoIs of one 10 x 5 x 5 grid with the same ``npos`` observed cells and seeds of their own"""
    hits = np.arange(250)[7::12][:npos]
    assert len(hits) == npos
    c = ref._scene([(10, 5, 5)] * n_seeds, [hits] * n_seeds, [1] * n_seeds, [0] * n_seeds,
                   [ref.row_seed(1234, s, 0) for s in range(n_seeds)])
    return c, hits


def test_the_draw_is_uniform():
    """10 x 5 x 5 cells, 20 observed, 512 row seeds: every free cell is drawn Binomial(512, 20 / 230) times, every list
    position survives cap = 10 of 40 Binomial(512, 1 / 4) times; each count within 6 standard deviations of its mean (a
    bound from the distribution: for 230 + 40 counts the chance that a fair draw misses it is below 1e-6)"""
    n = 512
    c, hits = _uniform_scene(n, 20)
    xyz, labels, index, _, counts = [a.numpy() if torch.is_tensor(a) else a for a in _aten(c, balance=True, cap=-1)]
    assert counts == [40] * n
    ids = ref.cell_ids(c, xyz, index)
    drawn = np.bincount(ids[labels == 0], minlength=250)
    free = np.setdiff1d(np.arange(250), hits)
    p = 20 / 230
    mean, sd = n * p, math.sqrt(n * p * (1 - p))
    assert drawn[hits].sum() == 0 and drawn[free].sum() == 20 * n
    print(f'free cells drawn {drawn[free].min()} .. {drawn[free].max()} times, mean {mean:.1f}, sd {sd:.2f}')
    assert (np.abs(drawn[free] - mean) <= 6 * sd).all()
    # the cap draw: which of the 40 list positions survive
    capped = [a.numpy() if torch.is_tensor(a) else a for a in _aten(c, balance=True, cap=10)]
    assert capped[4] == [10] * n
    survive = np.zeros(40, dtype=np.int64)
    cids = ref.cell_ids(c, capped[0], capped[2])
    for r in range(n):
        full_r = ids[index == r]
        pos = np.searchsorted(full_r, cids[capped[2] == r])              # cells are distinct here: npos <= nneg
        assert np.array_equal(full_r[pos], cids[capped[2] == r])
        survive[pos] += 1
    mean, sd = n / 4, math.sqrt(n * 0.25 * 0.75)
    print(f'list positions kept {survive.min()} .. {survive.max()} times, mean {mean:.1f}, sd {sd:.2f}')
    assert survive.sum() == 10 * n and (np.abs(survive - mean) <= 6 * sd).all()


def test_equal_keys_go_by_cell_index(tie):
    """a row seed under which two free cells of a 27 000-cell RoI carry one 32-bit key, the draw ending between them: the
    smaller index is drawn, the larger is not -- in the restatement and in the chain"""
    c1, c2 = tie.tie
    s = int(tie.row_seeds[0])
    assert c1 < c2 and ref.key(s, [c1])[0] == ref.key(s, [c2])[0]
    assert c1 not in tie.hits[0] and c2 not in tie.hits[0]
    for out in (ref.run_case(tie), _aten(tie)):
        xyz, labels, index = [a.numpy() if torch.is_tensor(a) else a for a in out[:3]]
        free = ref.cell_ids(tie, xyz, index)[labels == 0]
        assert c1 in free and c2 not in free and len(free) == len(tie.hits[0])
    k = int(np.prod(ref.TIE_DIMS))
    keys = ref.key(s, np.arange(k))
    obs = np.zeros(k, dtype=np.uint8)
    obs[tie.hits[0]] = 1
    rank = int(((keys < keys[c1]) & (obs == 0)).sum())
    assert rank + 1 == len(tie.hits[0])                                      # (t, c1) is the last free cell drawn


def test_mixer_matches_the_integers_of_the_package():
    from objectcentricocccompletion_amd.occ import occ_ops
    for seed, slot, frame in ((0, 0, 0), (7, 3, 250), (-5, 63, 4095), (2 ** 63 - 1, 2 ** 20, 2 ** 31 - 1)):
        assert occ_ops.tune_row_seed(seed, slot, frame) == ref.row_seed(seed, slot, frame)
    assert ref.mix64_int(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF         # splitmix64: the first output of seed 0
    s = torch.tensor([ref.row_seed(0, 1, 2)] * 5)
    c = torch.tensor([0, 1, 1023, 26999, 2 ** 30])
    got = occ_ops._tune_key(s, c).numpy().astype(np.uint64)
    assert np.array_equal(got, ref.key(int(s[0]), c.numpy()))


def test_argument_checks():
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ import occ_ops
    c = ref.mixed_scene(8)
    sizes, dims, start, total, v, xyz, roi, seeds, keep = _args(c)
    for fn in (occ_ops.tune_sample_aten, occ_ops.tune_sample):
        with pytest.raises(L.OcoccError, match='cap > 0 with balance == 0'):
            fn(sizes, dims, start, total, v, xyz, roi, seeds, keep, balance=False, cap=8)
        with pytest.raises(L.OcoccError, match='row_seeds'):
            fn(sizes, dims, start, total, v, xyz, roi, seeds.int(), keep)
        with pytest.raises(L.OcoccError, match='row_seeds'):
            fn(sizes, dims, start, total, v, xyz, roi, seeds[:-1], keep)
        with pytest.raises(L.OcoccError, match='row_keep'):
            fn(sizes, dims, start, total, v, xyz, roi, seeds, keep.long())
        with pytest.raises(L.OcoccError, match='start int64'):
            fn(sizes, dims.long(), start, total, v, xyz, roi, seeds, keep)
        with pytest.raises(L.OcoccError, match='local_xyz'):
            fn(sizes, dims, start, total, v, xyz[:, :2], roi, seeds, keep)
    with pytest.raises(L.OcoccError, match='prefix table'):
        occ_ops.tune_sample_aten(sizes, dims, start, total - 1, v, xyz, roi, seeds, keep)
    with pytest.raises(L.OcoccError, match='CPU tensor'):                     # the kernels have no host fallback of their own
        occ_ops.tune_sample(sizes, dims, start, total, v, xyz, roi, seeds, keep)
    empty = occ_ops.tune_sample_aten(sizes[:0], dims[:0], start[:1], 0, v, xyz[:0], roi[:0], seeds[:0], keep[:0])
    assert empty[4] == [] and empty[0].shape == (0, 3)


def test_switch_selects_the_chain(monkeypatch):
    from objectcentricocccompletion_amd.occ import occ_ops
    c = ref.mixed_scene(8)
    monkeypatch.setattr(occ_ops, 'TUNE_SAMPLE_KERNEL', False)
    _assert_equal(occ_ops.tune_sample(*_args(c), balance=True, cap=73), ref.run_case(c, True, 73))


def test_exports_are_declared_bound_and_documented():
    from objectcentricocccompletion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ococc_hip.h')).read()
    assert 'occ_ae_head.py:65-201' in header
    plain = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in EXPORTS:
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, plain)
        assert m, f'{name} is not declared in ococc_hip.h'
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1])
        assert hasattr(lib, name) and hasattr(_lib.lib, name)
        assert any(f'`{name}`' in line and line.startswith('|') for line in integration.splitlines()), name
    assert 'tune_sample.hip' in open(os.path.join(ROOT, 'objectcentricocccompletion_amd', 'csrc', 'Makefile')).read()
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'OCOCC_TUNE_SAMPLE_KERNEL' in readme and 'online_step_tuning' in readme
    # refusals come back as the library's error code before anything is dereferenced or launched
    count, fill = _lib.lib.ococc_tune_sample_count, _lib.lib.ococc_tune_sample_fill
    assert count(None, 8, None, 1, None, None, 0, 4, None, None, None) == -1
    assert b'cap > 0 with balance == 0' in _lib.lib.ococc_last_error()
    assert count(None, 8, None, -1, None, None, 1, 4, None, None, None) == -1
    assert count(None, 8, None, 1, None, None, 1, 4, None, None, None) == -1 and b'null pointer' in _lib.lib.ococc_last_error()
    assert count(None, 0, None, 0, None, None, 1, 4, None, None, None) == 0
    assert fill(None, 8, None, 1, None, None, 0.0, None, None, None, None, None, None, None, 4, None) == -1
    assert b'voxel_size' in _lib.lib.ococc_last_error()
    assert fill(None, 8, None, 1, None, None, 0.2, None, None, None, None, None, None, None, 4, None) == -1
    assert fill(None, 8, None, 1, None, None, 0.2, None, None, None, None, None, None, None, 0, None) == 0   # no rows
