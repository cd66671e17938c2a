"""Generate tests/golden/occ_merge.npz: the REFERENCE's own LoadPointsAndOccPredFromFile and LoadOccPredFromFile
(mmdet3d/datasets/pipelines/occ_pinelines.py:585-806) run on a small seeded cloud and its completed-occupancy files,
where the reference tree exists.  The two classes are imported from their own file through oracle/ref_shim.py, as
oracle/gen_golden_pipelines.py reaches occ_pinelines.py; stood in are only the base class's file reading (np.fromfile)
and, through gen_golden_pipelines.load_pipelines, the registry -- the points wrapper is the reference's own LiDARPoints.
Data only, no reference source.

The file holds the inputs (`cloud` [300, 6], `cells` [260, 4] with scores between 0.05 and 0.95, `cells_obj` [90, 4] the
one object file of the directory), `cases`, a JSON list of the settings, and per case `<name>/points`, the array the
reference returned, and `<name>/next_rand`, the next torch.rand(1) after the call under the case's seed: the position of
the filter_prob draw in the random-number call order.

usage: python tools/gen_golden_occ_merge.py"""
import json
import os
import sys
import tempfile
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim as R  # noqa: E402
from oracle.gen_golden_pipelines import load_pipelines  # noqa: E402

SEED = 17
# name, class, where the cells are (file / dir / missing), constructor arguments
CASES = [
    dict(name='file_thr_none', cls='both', src='file', kw=dict(points_use_dim=5, score_threshold=0.0)),
    dict(name='file_thr_some', cls='both', src='file', kw=dict(points_use_dim=5, score_threshold=0.5)),
    dict(name='file_thr_all', cls='both', src='file', kw=dict(points_use_dim=5, score_threshold=2.0)),
    dict(name='dir_dim5', cls='both', src='dir', kw=dict(points_use_dim=5, score_threshold=0.3)),
    dict(name='dir_dim3', cls='both', src='dir', kw=dict(points_use_dim=3, score_threshold=0.0)),
    dict(name='file_dim3_list', cls='both', src='file', kw=dict(points_use_dim=[0, 1, 2], score_threshold=0.5)),
    dict(name='missing_file', cls='both', src='missing_file', kw=dict(points_use_dim=5)),
    dict(name='missing_dir', cls='both', src='missing_dir', kw=dict(points_use_dim=3)),
    dict(name='filter_prob_1', cls='both', src='file', kw=dict(points_use_dim=5, score_threshold=0.5, filter_prob=1.0)),
    dict(name='filter_prob_0', cls='both', src='file', kw=dict(points_use_dim=5, score_threshold=0.5, filter_prob=0.0)),
    dict(name='tanh', cls='both', src='file', kw=dict(points_use_dim=5, score_threshold=0.5, tanh_dim=[3, 4])),
    dict(name='tanh_missing', cls='both', src='missing_file', kw=dict(points_use_dim=5, tanh_dim=[3, 4])),
    dict(name='after_load_file', cls='occ', src='file', dim=5, kw=dict(score_threshold=0.5)),
    dict(name='after_load_dir_dim3', cls='occ', src='dir', dim=3, kw=dict(score_threshold=0.0)),
    dict(name='after_load_all', cls='occ', src='file', dim=5, kw=dict(score_threshold=2.0)),
    dict(name='after_load_missing', cls='occ', src='missing_dir', dim=5, kw=dict()),
]


def inputs():
    rng = np.random.default_rng(SEED)
    cloud = np.concatenate([rng.normal(0, 25, (300, 3)), rng.random((300, 2)) * 3, rng.random((300, 1))], 1).astype(np.float32)
    cells = np.concatenate([rng.normal(0, 25, (260, 3)), 0.05 + 0.9 * rng.random((260, 1))], 1).astype(np.float32)
    cells[:4, 3] = np.float32(0.5) + np.array([0, 1, -1, 2], np.float32) * np.spacing(np.float32(0.5))   # at the threshold
    cells_obj = np.concatenate([rng.normal(0, 25, (90, 3)), np.full((90, 1), 0.62)], 1).astype(np.float32)
    cells_obj[45:, 3] = 0.21
    return cloud, cells, cells_obj


def write_tree(root, cloud, cells, cells_obj):
    """the files of one frame below ``root``; {src: occ_pred_filename} and the cloud's path"""
    os.makedirs(os.path.join(root, 'seg', '1000'))
    cloud.tofile(os.path.join(root, 'cloud.bin'))
    cells.tofile(os.path.join(root, 'seg', '1000.bin'))
    cells_obj.tofile(os.path.join(root, 'seg', '1000', '1_obj.bin'))
    src = dict(file=os.path.join(root, 'seg', '1000.bin'), dir=os.path.join(root, 'seg', '1000'),
               missing_file=os.path.join(root, 'seg', '2000.bin'), missing_dir=os.path.join(root, 'seg', '2000'))
    return src, os.path.join(root, 'cloud.bin')


class FileReader(object):
    """stands in for LoadPointsFromFile, of which the two classes use _load_points alone"""

    def _load_points(self, pts_filename):
        if not os.path.exists(pts_filename):
            raise FileNotFoundError(pts_filename)
        return np.fromfile(pts_filename, dtype=np.float32)


def main():
    _, _, LiDARPoints, _ = load_pipelines()
    import types
    for name, attrs in (('mmdet3d.datasets.pipelines', ('LoadPointsFromFile',)),
                        ('mmdet3d.datasets.pipelines.formating', ('DefaultFormatBundle3D',)),
                        ('mmdet3d.datasets.pipelines.transforms_3d', ('ObjectNameFilter', 'ObjectRangeFilter', 'RandomFlip3D'))):
        m = sys.modules.get(name)
        if m is None:
            m = types.ModuleType(name)
            sys.modules[name] = m
        for a in attrs:
            setattr(m, a, FileReader if a == 'LoadPointsFromFile' else object)
    op = R.load('mmdet3d.datasets.pipelines.occ_pinelines')
    cloud, cells, cells_obj = inputs()
    out = dict(cloud=cloud, cells=cells, cells_obj=cells_obj, cases=np.array(json.dumps(CASES)), seed=np.array(SEED))
    with tempfile.TemporaryDirectory() as root, warnings.catch_warnings():
        warnings.simplefilter('ignore')
        src, cloud_path = write_tree(root, cloud, cells, cells_obj)
        for c in CASES:
            results = dict(occ_pred_filename=src[c['src']], pts_filename=cloud_path)
            torch.manual_seed(SEED)
            if c['cls'] == 'both':
                got = op.LoadPointsAndOccPredFromFile('LIDAR', points_load_dim=6, occs_load_dim=4, **c['kw'])(results)
            else:
                pts = torch.from_numpy(np.ascontiguousarray(cloud[:, :c['dim']]))
                results['points'] = LiDARPoints(pts, points_dim=c['dim'], attribute_dims=None)
                got = op.LoadOccPredFromFile('LIDAR', occs_load_dim=4, **c['kw'])(results)
            arr = got['points'].tensor.numpy().copy()
            assert arr.dtype == np.float32, (c['name'], arr.dtype)
            out[c['name'] + '/points'] = arr
            out[c['name'] + '/next_rand'] = torch.rand(1).numpy()
    by = {c['name']: out[c['name'] + '/points'] for c in CASES}
    # the branches are the ones the names claim
    assert len(by['file_thr_none']) == 300 + 260 and len(by['file_thr_all']) == 300 and 300 < len(by['file_thr_some']) < 560
    assert len(by['filter_prob_1']) == len(by['file_thr_some']) and len(by['filter_prob_0']) == 560
    assert len(by['dir_dim5']) == 300 + 45 and len(by['dir_dim3']) == 300 + 90 and by['dir_dim3'].shape[1] == 5
    assert len(by['missing_file']) == len(by['missing_dir']) == 300
    assert not np.array_equal(out['missing_file/next_rand'], out['file_thr_none/next_rand'])   # no draw without cells
    assert not np.array_equal(by['tanh'][:300, 3:5], by['file_thr_some'][:300, 3:5])
    path = os.path.join(ROOT, 'tests', 'golden', 'occ_merge.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes', {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
