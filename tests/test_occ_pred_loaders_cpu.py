"""pipelines.LoadPointsAndOccPredFromFile and LoadOccPredFromFile against what the reference's own two classes returned
(tests/golden/occ_merge.npz, written by tools/gen_golden_occ_merge.py): single file and directory, a missing path, a
threshold above all, some and none of the scores, points_use_dim 3 and 5, filter_prob 1.0 and 0.0 under a fixed seed,
tanh_dim, and LoadOccPredFromFile after a plain load.  Exact, except the tanh columns (4 f32 ulp: np.tanh may take
another vector path on another CPU; nothing else in these loaders computes).  And occ_export.occ_pred_filename."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from objectcentricocccompletion_amd import occ_export, pipelines
from objectcentricocccompletion_amd.registry import PIPELINES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, 'tests', 'golden', 'occ_merge.npz'))
CASES = json.loads(str(GOLDEN['cases']))


@pytest.fixture(scope='module', autouse=True)
def _generator_as_found():
    cpu = torch.get_rng_state()
    yield
    torch.set_rng_state(cpu)


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    """the files of the golden's one frame: {src: occ_pred_filename}, the cloud's path"""
    root = str(tmp_path_factory.mktemp('occ_merge'))
    os.makedirs(os.path.join(root, 'seg', '1000'))
    GOLDEN['cloud'].tofile(os.path.join(root, 'cloud.bin'))
    GOLDEN['cells'].tofile(os.path.join(root, 'seg', '1000.bin'))
    GOLDEN['cells_obj'].tofile(os.path.join(root, 'seg', '1000', '1_obj.bin'))
    src = dict(file=occ_export.occ_pred_filename(root, 'seg', 1000, False), dir=occ_export.occ_pred_filename(root, 'seg', 1000, True),
               missing_file=occ_export.occ_pred_filename(root, 'seg', 2000, False),
               missing_dir=occ_export.occ_pred_filename(root, 'seg', 2000, True))
    return src, os.path.join(root, 'cloud.bin')


def _ulps(a, b):
    """distance in f32 ulp of b"""
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_loader_reproduces_the_reference(c, tree):
    src, cloud_path = tree
    results = dict(occ_pred_filename=src[c['src']], pts_filename=cloud_path)
    torch.manual_seed(int(GOLDEN['seed']))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if c['cls'] == 'both':
            step = PIPELINES.build(dict(type='LoadPointsAndOccPredFromFile', coord_type='LIDAR', points_load_dim=6,
                                        occs_load_dim=4, **c['kw']))
        else:
            results['points'] = np.ascontiguousarray(GOLDEN['cloud'][:, :c['dim']])
            step = PIPELINES.build(dict(type='LoadOccPredFromFile', coord_type='LIDAR', occs_load_dim=4, **c['kw']))
        out = step(results)
    assert out is results and {'occ_pred_filename', 'pts_filename', 'points'} <= set(out)
    got, want = out['points'], GOLDEN[c['name'] + '/points']
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == want.shape
    tanh = c['kw'].get('tanh_dim') or []
    exact = [j for j in range(want.shape[1]) if j not in tanh]
    assert got[:, exact].tobytes() == want[:, exact].tobytes()
    if tanh:
        n = len(GOLDEN['cloud'])
        assert got[n:, tanh].tobytes() == want[n:, tanh].tobytes()             # the cells' zeros
        worst = float(_ulps(got[:n, tanh], want[:n, tanh]).max())
        print(f'{c["name"]}: tanh columns within {worst:.2f} ulp of the recorded ones')
        assert worst <= 4.0
        assert not np.array_equal(want[:n, tanh], GOLDEN['cloud'][:, tanh])   # (tanh was applied)
    # the filter_prob draw sits where the reference makes it: the generator is where the reference left it
    assert torch.rand(1).numpy().tobytes() == GOLDEN[c['name'] + '/next_rand'].tobytes()


def test_golden_branches_are_the_ones_named():
    by = {c['name']: GOLDEN[c['name'] + '/points'] for c in CASES}
    n, m = len(GOLDEN['cloud']), len(GOLDEN['cells'])
    assert len(by['file_thr_none']) == n + m and len(by['file_thr_all']) == n and n < len(by['file_thr_some']) < n + m
    assert len(by['filter_prob_0']) == n + m and len(by['filter_prob_1']) == len(by['file_thr_some'])
    # strict compare at the threshold: of the four cells at 0.5 + {0, 1, -1, 2} ulp, the second and fourth are kept
    kept = by['file_thr_some'][n:]
    assert [bool((kept[:, :3] == GOLDEN['cells'][i, :3]).all(1).any()) for i in range(4)] == [False, True, False, True]
    assert (by['file_thr_some'][:n, -2:] == 0).all() and (kept[:, -1] == 1).all() and (kept[:, 3:5] == 0).all()
    assert by['dir_dim3'].shape == (n + len(GOLDEN['cells_obj']), 5) and len(by['dir_dim5']) == n + 45
    assert by['after_load_file'].tobytes() == by['file_thr_some'].tobytes()
    assert not np.array_equal(GOLDEN['missing_file/next_rand'], GOLDEN['file_thr_none/next_rand'])


def test_directory_is_read_in_sorted_order(tmp_path):
    """two object files: the cells of the first name come first, whatever order they were written in"""
    d = tmp_path / 'seg' / '7'
    d.mkdir(parents=True)
    a, b = np.full((2, 4), 1, np.float32), np.full((3, 4), 2, np.float32)
    b.tofile(str(d / '2_b.bin'))
    a.tofile(str(d / '1_a.bin'))
    np.zeros((1, 6), np.float32).tofile(str(tmp_path / 'cloud.bin'))
    out = pipelines.LoadPointsAndOccPredFromFile('LIDAR', points_use_dim=3)(
        dict(occ_pred_filename=str(d), pts_filename=str(tmp_path / 'cloud.bin')))
    assert out['points'][:, 0].tolist() == [0, 1, 1, 2, 2, 2] and out['points'][:, -1].tolist() == [0, 1, 1, 1, 1, 1]
    with pytest.raises(AssertionError):
        pipelines.LoadPointsAndOccPredFromFile('LIDAR', points_load_dim=4, points_use_dim=5)
    with pytest.raises(AssertionError):
        pipelines.LoadOccPredFromFile('RADAR')


def test_occ_pred_filename():
    assert occ_export.occ_pred_filename('/data/occ', 'segment-1', 1553629304279740, False) == '/data/occ/segment-1/1553629304279740.bin'
    assert occ_export.occ_pred_filename('/data/occ', 'segment-1', 1553629304279740, True) == '/data/occ/segment-1/1553629304279740'
    # the per-object name is the directory occ_path writes into
    assert os.path.dirname(occ_export.occ_path('/data/occ', 'segment-1', 7, 1, 'abc')) == occ_export.occ_pred_filename(
        '/data/occ', 'segment-1', 7, True)
