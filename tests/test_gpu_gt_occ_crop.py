"""Ground-truth occupancy export on the MI355X (csrc/gt_occ_crop.hip): bbox.crop_gt_occ_packed against the
operator-by-operator crop_gt_occ_aten bit for bit (points, order, counts, value column) over the tile and round edges,
the faces of the box, TrackletRoIHeadOCC.save_gt_occ_from_tracklet and tools/test.py --save-gt-occ."""
import ast
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gt_occ_ref import face_case, random_case                                  # noqa: E402
from test_gpu_occ_export import CFG, _listing, _run, _tracklet                 # noqa: E402 (the tiny tracklet of that test)


def _check(cells, gt, roi, values=None, trig=None):
    """kernels == torch.cat(comparator): points, order, counts and the value column; -> (packed, counts)"""
    from objectcentricocccompletion_amd import bbox
    exp = bbox.crop_gt_occ_aten(cells, gt, roi, trig)
    if trig is not None:
        got, counts = bbox.gt_occ_crop_kernels(cells, gt, roi, *trig, values=values)
    else:
        got, counts = bbox.crop_gt_occ_packed(cells, gt, roi, values)
    N = gt.size(0)
    assert len(exp) == N and counts == [int(t.size(0)) for t in exp]
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (sum(counts), 4)
    if N:
        assert torch.equal(got[:, :3], torch.cat(exp))
        col = values if values is not None else torch.ones(N, device=got.device)
        assert torch.equal(got[:, 3], col.repeat_interleave(torch.tensor(counts, device=got.device)))
    return got, counts


@pytest.mark.parametrize('N', [0, 1, 3])
def test_packed_equals_the_comparator_over_round_and_tile_edges(dev, N):
    for K in (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049):
        cells, gt, roi = random_case(N, K, seed=100 * N + K % 97, dev=dev)
        values = torch.linspace(0.25, 0.75, N, device=dev) if K % 2 else None
        _, counts = _check(cells, gt, roi, values)
        if N and K >= 63:
            assert 0 < sum(counts) < N * K, (N, K, counts)                      # the crop keeps some and drops some


@pytest.mark.parametrize('N', [2047, 2048, 2049])
def test_packed_equals_the_comparator_with_many_frames(dev, N):
    cells, gt, roi = random_case(N, 3, seed=N, dev=dev)
    _, counts = _check(cells, gt, roi, torch.rand(N, generator=torch.Generator().manual_seed(1)).to(dev))
    assert 0 < sum(counts) < 3 * N


def test_far_roi_enclosing_roi_strided_boxes_and_repeatability(dev, monkeypatch):
    from objectcentricocccompletion_amd import bbox
    cells, gt, roi = random_case(5, 1500, seed=9, dev=dev)
    roi[2, :2] += 500.0                                                         # a frame in the middle keeps nothing
    got, counts = _check(cells, gt, roi)
    assert counts[2] == 0 and all(c > 0 for i, c in enumerate(counts) if i != 2)
    # rows of a wider tensor (what gt_rois[:, 1:] of the RoI head is): the row stride is passed on, not copied away
    wide_g, wide_r = torch.cat([torch.ones(5, 1, device=dev), gt], 1), torch.cat([roi, torch.zeros(5, 2, device=dev)], 1)
    again, again_counts = _check(cells, wide_g[:, 1:], wide_r[:, :7])
    assert again_counts == counts and got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    twice, _ = bbox.crop_gt_occ_packed(cells, gt, roi)                          # two runs: identical bytes
    assert got.cpu().numpy().tobytes() == twice.cpu().numpy().tobytes()
    # the switch: the ATen chain, the same bytes, the kernels not reached
    monkeypatch.setattr(bbox, 'GT_OCC_KERNEL', False)
    monkeypatch.setattr(bbox, 'gt_occ_crop_kernels', None)
    aten, aten_counts = bbox.crop_gt_occ_packed(cells, gt, roi)
    assert aten_counts == counts and got.cpu().numpy().tobytes() == aten.cpu().numpy().tobytes()
    monkeypatch.undo()
    # an RoI that encloses every cell
    big = gt.clone()
    big[:, 3:6] = 20.0
    big[:, 2] -= 8.0
    _, counts = _check(cells, gt, big, torch.full((5,), 0.5, device=dev))
    assert counts == [1500] * 5


def test_cells_on_the_faces(dev):
    cells, gt, roi, trig, keep = face_case(dev)
    got, counts = _check(cells, gt, roi, trig=trig)
    exp = (cells + torch.tensor([8.0, -4.0, 2.0], device=dev))[torch.tensor(keep, device=dev)]
    assert counts == [sum(keep)] and torch.equal(got[:, :3], exp) and bool((got[:, 3] == 1).all())


def test_env_switch_is_read_at_import():
    import objectcentricocccompletion_amd.bbox as bbox
    assert bbox.GT_OCC_KERNEL == (os.environ.get('OCOCC_GT_OCC_KERNEL', '1') != '0')


# ------------------------------------------------------------------------------------------------ the RoI head, files
@pytest.fixture(scope='module')
def model(dev):
    from objectcentricocccompletion_amd import config, dataset, heads, point_pool, roi_head  # noqa: F401
    from objectcentricocccompletion_amd.registry import DETECTORS
    torch.manual_seed(0)
    return DETECTORS.build(config.fromfile(CFG)['model']).to(dev).eval()


def test_save_gt_occ_from_tracklet(dev, model, tmp_path, monkeypatch, capsys):
    from objectcentricocccompletion_amd import bbox, occ_export
    from objectcentricocccompletion_amd.tracklet import Tracklet
    head = model.roi_head
    trk = _tracklet(dev)                                                        # 5 frames
    matched = [0, 2, 3]                                                         # 3 of them have a GT box
    g = torch.Generator().manual_seed(6)
    gt_boxes = trk.boxes[matched, :7].cpu() + torch.cat([torch.rand(3, 3, generator=g) * 0.6 - 0.3,
                                                         torch.rand(3, 3, generator=g) * 0.2,
                                                         torch.rand(3, 1, generator=g) * 0.2 - 0.1], 1)
    gt = Tracklet(gt_boxes.to(dev), [trk.ts_list[i] for i in matched], torch.ones(3, device=dev), type=1,
                  segment_name=trk.segment_name, id='obj_7')
    gt_rois = head.get_gt_rois([trk], [gt])
    assert gt_rois[:, 0].tolist() == [1.0, 0.0, 1.0, 1.0, 0.0]
    xyz = (torch.rand(900, 3, generator=g) * 2 - 1) * torch.tensor([1.3, 2.7, 1.0])
    label = torch.randint(0, 3, (900, 1), generator=g).float()                  # 0 free, 1 occupied, 2 unknown
    occ = torch.cat([xyz, label], 1).to(dev)
    cells = occ[:, :3][occ[:, 3] == 1]
    rois = head.tracklets2rois([trk])[0]
    exp = bbox.crop_gt_occ_aten(cells, gt_rois[matched][:, 1:], rois[matched][:, 1:8])
    assert 0 < sum(int(t.size(0)) for t in exp) < 3 * cells.size(0)
    res = dict(nonempty_roi_mask=torch.tensor([True, True, True, False, True], device=dev))
    name = lambda i: os.path.join(trk.segment_name, str(trk.ts_list[i]), '1_obj_7.bin')

    def check(root, frames):
        assert _listing(root) == sorted(name(i) for i in frames)
        for i in frames:
            a = occ_export.read_occ_bin(os.path.join(root, name(i)))
            e = exp[matched.index(i)].cpu().numpy()
            assert a.dtype == np.float32 and a.shape == (e.shape[0], 4)
            assert np.array_equal(a[:, :3], e) and np.all(a[:, 3] == 1)

    root = str(tmp_path / 'all')
    monkeypatch.setitem(head.test_cfg, 'gt_occ_save_root', root)
    paths = head.save_gt_occ_from_tracklet([trk], res, gt_rois, [occ])
    assert [os.path.relpath(p, root) for p in paths] == [name(i) for i in matched]
    check(root, matched)
    other = str(tmp_path / 'other')                                             # root= overrides the config's directory
    head.save_gt_occ_from_tracklet([trk], res, gt_rois, [occ], root=other)
    check(other, matched)
    # min_evaluate_length and filter_empty_roi go by the frame's index in the PROPOSAL tracklet: frame 0 is under the
    # length, frame 3 is the RoI without points
    root = str(tmp_path / 'filtered')
    monkeypatch.setitem(head.test_cfg, 'gt_occ_save_root', root)
    monkeypatch.setitem(head.test_cfg, 'min_evaluate_length', 1)
    monkeypatch.setitem(head.test_cfg, 'filter_empty_roi', True)
    capsys.readouterr()
    head.save_gt_occ_from_tracklet([trk], res, gt_rois, [occ])
    assert f'empty roi 3 in {trk.segment_name} at {trk.ts_list[3]}' in capsys.readouterr().out
    check(root, [2])
    # nothing to write: no labels, no matched frame, no occupied cell
    root = str(tmp_path / 'none')
    monkeypatch.setitem(head.test_cfg, 'gt_occ_save_root', root)
    no_match = gt_rois.clone()
    no_match[:, 0] = 0
    free = occ.clone()
    free[:, 3] = 0
    assert head.save_gt_occ_from_tracklet([trk], res, gt_rois, [None]) == []
    assert head.save_gt_occ_from_tracklet([trk], res, gt_rois, None) == []
    assert head.save_gt_occ_from_tracklet([trk], res, None, [occ]) == []
    assert head.save_gt_occ_from_tracklet([trk], res, no_match, [occ]) == []
    assert head.save_gt_occ_from_tracklet([trk], res, gt_rois, [free]) == []
    assert _listing(root) == []
    with pytest.raises(AssertionError):
        head.save_gt_occ_from_tracklet([trk, trk], res, gt_rois, [occ])


def test_tools_test_save_gt_occ(dev, model, tmp_path):
    """tools/test.py --eval iou --save-gt-occ DIR in a child process: one file per tracklet and frame with a GT box,
    holding what the comparator gives, and the occupancy IoU of the same command without the flag (a second child
    process: no state of the test process enters the comparison)."""
    from objectcentricocccompletion_amd import bbox, config, occ_export
    from objectcentricocccompletion_amd.pipelines import collate_tracklets
    from objectcentricocccompletion_amd.registry import DATASETS
    data, ckpt, out = str(tmp_path / 'data'), str(tmp_path / 'model.pth'), str(tmp_path / 'gt_occ')
    _run([sys.executable, 'tools/make_synthetic_dataset.py', data, '--tracklets', '2', '--frames', '12'])
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    cmd = ['timeout', '-k', '10', '300', sys.executable, 'tools/test.py', CFG, ckpt, '--data-root', data, '--eval', 'iou']
    metrics = lambda stdout: ast.literal_eval([l for l in stdout.strip().splitlines() if l.startswith('{')][-1])
    got, plain = metrics(_run(cmd + ['--save-gt-occ', out])), metrics(_run(cmd))
    print('with the flag', got, 'without', plain)
    assert got == plain and 'iou' in got                                        # the numbers of the run without the flag
    cfg = config.fromfile(CFG)
    j = lambda p: os.path.join(data, p)
    ds = DATASETS.build(dict(cfg['data']['test'], data_root=data, ann_file=j('tracklet_data/synth_training_gt_candidates.pkl'),
                             tracklet_proposals_file=j('tracklet_data/synth_training.pkl'), occ_anno_root=j('occ_gt'),
                             pose_file=j('poses.pkl')))
    head = model.roi_head
    assert 'save_gt_occ' not in head.test_cfg
    expected, frames_total = {}, 0
    with torch.no_grad():
        for i in range(len(ds)):
            np.random.seed(i)
            torch.manual_seed(i)
            batch = collate_tracklets([ds[i]], dev)
            trk = batch['tracklet'][0]                                          # the tracklet the RoI head is given
            gts, occs, _ = head._select_one2one_candidates(batch['tracklet'], batch['gt_tracklet_candidates'],
                                                           batch['occ_labels'], batch['occ_labels_scores'])
            gt_rois = head.get_gt_rois(batch['tracklet'], gts)
            frames = [f for f, m in enumerate(gt_rois[:, 0].tolist()) if m == 1]
            frames_total += len(trk)
            if occs[0] is not None and frames:
                cells = occs[0][..., :3][occs[0][..., 3] == 1]
                rois = head.tracklets2rois([trk])[0]
                parts = bbox.crop_gt_occ_aten(cells, gt_rois[frames][:, 1:], rois[frames][:, 1:8]) if cells.size(0) else []
                for f, p in zip(frames, parts):
                    expected[os.path.join(str(trk.segment_name), str(trk.ts_list[f]), f'{trk.type}_{trk.id}.bin')] = p
    print(f'{len(expected)} files for {frames_total} frames')
    assert len(ds) == 2 and 0 < len(expected) <= frames_total and _listing(out) == sorted(expected)
    rows = 0
    for rel, p in expected.items():
        a = occ_export.read_occ_bin(os.path.join(out, rel))
        assert a.shape == (p.size(0), 4) and np.array_equal(a[:, :3], p.cpu().numpy()) and np.all(a[:, 3] == 1)
        rows += a.shape[0]
    assert rows > 0
