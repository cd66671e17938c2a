"""Completed-occupancy export on the MI355X (csrc/occ_export.hip): the cells kernel against
occ_ops.dense_voxel_centers_batched, the selection kernels against the ATen chain of OccDecoder.get_occ, get_occ_packed
against get_occ and the reference's golden decode, TrackletRoIHeadOCC.save_occ_from_tracklet and tools/test.py --save-occ.
Everything but the golden comparison is bit for bit."""
import ast
import glob
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'ococcnet_mi355x.py')
V = 0.2
ENLARGE = [([1.0, 1.0, 1.0], [0.5, 0.5, 0.5]), ([1.2, 1.1, 1.0], [0.0, 0.0, 0.0])]
# the ENLARGED sizes of the six boxes: an exact multiple of the voxel on x (the ceil edge), a single cell, no cells (in
# the middle: the RoI search steps over it), more than 1024 cells (several tiles), more than 4096, an ordinary box
TARGET = [[2.0, 1.5, 1.4], [0.15, 0.1, 0.2], [0.0, 0.0, 0.0], [2.3, 2.1, 1.9], [6.1, 2.9, 2.3], [1.03, 0.77, 1.51]]


def _raw_sizes(scale, offset, dev, extra=()):
    """box sizes whose enlarged sizes are TARGET (+ extra) under (scale, offset); the enlargement itself is left to the
    code under test"""
    t = torch.tensor(TARGET + list(extra), dtype=torch.float32)
    return ((t - torch.tensor(offset)) / torch.tensor(scale)).to(dev)


def _layout(raw, scale, offset):
    from objectcentricocccompletion_amd.occ import occ_ops
    sizes, dims, start, total = occ_ops.dense_grid_layout(raw, V, scale, offset)
    k = dims.long().prod(1).tolist()
    assert k[1] == 1 and k[2] == 0 and 1024 < k[3] < 4096 < k[4] and total == sum(k)   # the cases are what they claim
    return sizes, dims, start, total


@pytest.mark.parametrize('enlarge', ENLARGE)
def test_cells_equal_dense_voxel_centers_batched(dev, enlarge):
    from objectcentricocccompletion_amd.occ import occ_ops
    scale, offset = enlarge
    raw = _raw_sizes(scale, offset, dev)
    exp_c, exp_box, exp_k = occ_ops.dense_voxel_centers_batched(raw, V, scale, offset)
    sizes, dims, start, total = _layout(raw, scale, offset)
    assert total == exp_c.size(0) and torch.equal(start[1:] - start[:-1], exp_k)
    if scale == [1.0, 1.0, 1.0]:
        assert float(sizes[0, 0]) == 2.0                      # 1.5 + 0.5: the size is an exact multiple of the voxel
    s = start.tolist()
    ranges = [(0, total),
              (s[3] + 500, s[4] + 3000),                      # from the middle of a tile of one RoI into the next RoI
              (s[4] + 100, s[4] + 2100),                      # starts and ends inside the same RoI
              (s[1], s[3] + 1), (total - 1, total), (7, 7)]   # over the RoI without cells; one cell; none
    for lo, hi in ranges:
        c, idx = occ_ops.dense_grid_cells(sizes, dims, start, V, lo, hi, total)
        assert c.dtype == torch.float32 and idx.dtype == torch.int32 and tuple(c.shape) == (hi - lo, 3)
        assert torch.equal(c, exp_c[lo:hi]), (lo, hi)
        assert torch.equal(idx.long(), exp_box[lo:hi]), (lo, hi)
    from objectcentricocccompletion_amd._lib import OcoccError
    with pytest.raises(OcoccError):
        occ_ops.dense_grid_cells(sizes, dims, start, V, 5, 4, total)
    with pytest.raises(OcoccError, match=f'of {total} cells'):
        occ_ops.dense_grid_cells(sizes, dims, start, V, 0, total + 1, total)       # past the last cell
    # no RoI at all
    e = occ_ops.dense_grid_layout(raw[:0], V, scale, offset)
    c, idx = occ_ops.dense_grid_cells(e[0], e[1], e[2], V, 0, 0, 0)
    assert e[3] == 0 and tuple(c.shape) == (0, 3) and tuple(idx.shape) == (0,)


def test_cells_more_rois_than_the_lds_table(dev):
    """R + 1 > 2048: the RoI search reads the prefix from global memory"""
    from objectcentricocccompletion_amd.occ import occ_ops
    g = torch.Generator().manual_seed(3)
    raw = (torch.rand(2100, 3, generator=g) * 0.9).to(dev)
    raw[::7] = -0.5                                             # RoIs without cells in between
    exp_c, exp_box, _ = occ_ops.dense_voxel_centers_batched(raw, V, *ENLARGE[0])
    sizes, dims, start, total = occ_ops.dense_grid_layout(raw, V, *ENLARGE[0])
    c, idx = occ_ops.dense_grid_cells(sizes, dims, start, V, 0, total, total)
    assert torch.equal(c, exp_c) and torch.equal(idx.long(), exp_box)


def test_cells_equal_the_golden_centres(dev, golden_dir):
    from objectcentricocccompletion_amd.occ import occ_ops
    gd = np.load(os.path.join(golden_dir, 'occ_decode.npz'))
    rois = torch.from_numpy(gd['rois']).to(dev)
    assert rois.size(0) == 7
    sizes, dims, start, total = occ_ops.dense_grid_layout(rois[:, 4:7], V, *ENLARGE[0])
    c, idx = occ_ops.dense_grid_cells(sizes, dims, start, V, 0, total, total)
    assert np.array_equal(c.cpu().numpy(), gd['centers'])
    assert np.array_equal(torch.bincount(idx.long(), minlength=7).cpu().numpy(), gd['cells_per_roi'])


# ------------------------------------------------------------------------------------------------ selection
def _selection_case(dev, pos_thresh):
    """the six grids, one more RoI whose logits are all negative and one whose logits are all positive"""
    from objectcentricocccompletion_amd.occ import occ_ops
    scale, offset = ENLARGE[0]
    raw = _raw_sizes(scale, offset, dev, extra=[[1.1, 0.9, 1.3], [0.9, 1.3, 0.7]])
    R = raw.size(0)
    g = torch.Generator().manual_seed(17)
    rois = torch.cat([torch.zeros(R, 1), torch.rand(R, 3, generator=g) * 80 - 40, raw.cpu(),
                      torch.rand(R, 1, generator=g) * 6.4 - 3.2], 1).to(dev)
    centers, box, k = occ_ops.dense_voxel_centers_batched(raw, V, scale, offset)
    N = centers.size(0)
    logits = torch.randn(N, generator=g) * 3
    thr = float(np.log(pos_thresh / (1 - pos_thresh)))
    t32 = np.float32(thr)
    near = torch.tensor([0.0, 1e-7, -1e-7, thr, np.nextafter(t32, np.float32(1)), np.nextafter(t32, np.float32(-1)),
                         float('nan'), float('inf'), float('-inf')], dtype=torch.float32)
    pick = torch.rand(N, generator=g) < 0.2
    logits[pick] = near[torch.randint(0, len(near), (int(pick.sum()),), generator=g)]
    logits[:3] = torch.tensor([0.0, 1e-7, -1e-7])
    logits = logits.to(dev)
    logits[box == R - 2] = -logits[box == R - 2].abs().nan_to_num(1.0) - 1.0
    logits[box == R - 1] = logits[box == R - 1].abs().nan_to_num(1.0) + 1.0
    return types.SimpleNamespace(raw=raw, rois=rois, centers=centers, box=box, k=k, logits=logits, R=R,
                                 scale=scale, offset=offset)


def _aten_select(c, pos_thresh, transform, roi_values=None, with_score=False):
    from objectcentricocccompletion_amd.occ.occ_base import OccDecoder
    sel = c.logits.sigmoid().view(-1) > pos_thresh
    pts, pbox = c.centers[sel], c.box[sel]
    if transform:
        pts = OccDecoder._to_lidar(pts, pbox, c.rois[:, 1:4], c.rois[:, 4:7], c.rois[:, 7])
    if roi_values is not None:
        pts = torch.cat([pts, roi_values[pbox].view(-1, 1)], 1)
    elif with_score:
        pts = torch.cat([pts, c.logits[sel].sigmoid().view(-1, 1)], 1)
    return pts, torch.bincount(pbox, minlength=c.R).tolist()


@pytest.mark.parametrize('pos_thresh', [0.5, 0.3])
def test_selection_equals_the_aten_chain(dev, pos_thresh):
    from objectcentricocccompletion_amd.occ import occ_ops
    c = _selection_case(dev, pos_thresh)
    sizes, dims, start, total = _layout(c.raw, c.scale, c.offset)
    assert total == c.logits.numel()
    values = torch.rand(c.R, generator=torch.Generator().manual_seed(5)).to(dev)
    for transform in (False, True):
        rois = c.rois if transform else None
        for kw, ref_kw in ((dict(), dict()), (dict(roi_values=values), dict(roi_values=values)),
                           (dict(with_score=True), dict(with_score=True))):
            exp, exp_counts = _aten_select(c, pos_thresh, transform, **ref_kw)
            got, counts = occ_ops.occ_select(c.logits.view(-1, 1), sizes, dims, start, total, V, pos_thresh, rois, **kw)
            assert counts == exp_counts and counts[2] == 0 and counts[-2] == 0 and counts[-1] == int(c.k[-1])
            assert got.dtype == torch.float32 and got.shape == exp.shape
            assert torch.equal(got, exp), (transform, sorted(kw))
            again, _ = occ_ops.occ_select(c.logits, sizes, dims, start, total, V, pos_thresh, rois, **kw)
            assert got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()      # two runs: identical bytes


def test_selection_without_rois_or_cells(dev):
    from objectcentricocccompletion_amd._lib import OcoccError
    from objectcentricocccompletion_amd.occ import occ_ops
    sizes, dims, start, total = occ_ops.dense_grid_layout(torch.ones(2, 3, device=dev), V)
    with pytest.raises(OcoccError, match=f'{total - 1} logits for a layout of {total} cells'):
        occ_ops.occ_select(torch.zeros(total - 1, device=dev), sizes, dims, start, total, V, 0.5)   # fewer logits than cells
    raw = torch.zeros(0, 3, device=dev)
    sizes, dims, start, total = occ_ops.dense_grid_layout(raw, V)
    pts, counts = occ_ops.occ_select(torch.zeros(0, device=dev), sizes, dims, start, total, V, 0.5)
    assert tuple(pts.shape) == (0, 3) and counts == []
    raw = torch.zeros(3, 3, device=dev)                                     # three RoIs, none has a cell
    sizes, dims, start, total = occ_ops.dense_grid_layout(raw, V)
    pts, counts = occ_ops.occ_select(torch.zeros(0, device=dev), sizes, dims, start, total, V, 0.5, with_score=True)
    assert total == 0 and tuple(pts.shape) == (0, 4) and counts == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ decoder, golden
@pytest.fixture(scope='module')
def golden_decoder(dev, golden_dir):
    """construction and weights of test_gpu_ococc.test_dense_grid_decode_vs_reference_golden"""
    from objectcentricocccompletion_amd.occ.occ_base import OccDecoder
    gd = np.load(os.path.join(golden_dir, 'occ_decode.npz'))
    dec = OccDecoder(256, [64, 128, 128], pos_encode_L=10, norm_cfg=dict(type='LN', eps=1e-3), act='gelu',
                     occ_dropout=0.0, use_ln=True)
    dec.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in dec.state_dict().items()}, seed=11))
    rois, feats = torch.from_numpy(gd['rois']).to(dev), torch.from_numpy(gd['feats']).to(dev)
    return dec.to(dev).eval(), gd, rois, feats


def test_get_occ_packed_equals_get_occ(dev, golden_decoder):
    dec, gd, rois, feats = golden_decoder
    S, O_ = ENLARGE[0]
    assert rois[:, 0].tolist() == sorted(rois[:, 0].tolist())                # get_occ's sample lists are in RoI order
    values = torch.linspace(0.1, 0.9, rois.size(0), device=dev)
    for transform in (True, False):
        per_roi = [t for s in dec.get_occ(feats, rois, V, S, O_, transform=transform) for t in s]
        exp = torch.cat(per_roi)
        assert exp.size(0) > 1000
        for kw in (dict(chunk=10000), dict()):
            got, counts = dec.get_occ_packed(feats, rois, V, S, O_, transform=transform, **kw)
            assert counts == [int(t.size(0)) for t in per_roi]
            assert torch.equal(got, exp), (transform, kw)
        got, counts = dec.get_occ_packed(feats, rois, V, S, O_, transform=transform, roi_values=values)
        assert torch.equal(got[:, :3], exp)
        assert torch.equal(got[:, 3], values.repeat_interleave(torch.tensor(counts, device=dev)))
    got, counts = dec.get_occ_packed(feats[:0], rois[:0], V, S, O_)
    assert tuple(got.shape) == (0, 3) and counts == []


def test_get_occ_packed_switch_takes_the_aten_chain(dev, golden_decoder, monkeypatch):
    from objectcentricocccompletion_amd.occ import occ_base, occ_ops
    dec, gd, rois, feats = golden_decoder
    S, O_ = ENLARGE[0]
    exp, exp_counts = dec.get_occ_packed(feats, rois, V, S, O_)
    monkeypatch.setattr(occ_base, 'OCC_EXPORT_KERNEL', False)
    monkeypatch.setattr(occ_ops, 'occ_select', None)                          # the kernels are not reached
    got, counts = dec.get_occ_packed(feats, rois, V, S, O_)
    assert counts == exp_counts and torch.equal(got, exp)


def test_get_occ_packed_vs_reference_golden(dev, golden_decoder):
    """Against the reference's own decode (tests/golden/occ_decode.npz).  The logits agree to 2e-3 only (f32 GEMMs in
    another order), so a cell whose reference logit is within 1e-3 of the threshold may fall on either side: 66 of the
    34 031 cells of the fixture.  Every other occupied cell of the reference is present, within 2e-5."""
    dec, gd, rois, feats = golden_decoder
    S, O_ = ENLARGE[0]
    lr = gd['logits'].reshape(-1)
    k = gd['cells_per_roi'].astype(np.int64)
    near = np.abs(lr) <= 1e-3
    assert lr.size == 34031 == int(k.sum()) and int(near.sum()) <= 66
    roi = np.repeat(np.arange(len(k)), k)
    near_per_roi = np.bincount(roi[near], minlength=len(k))
    got, counts = dec.get_occ_packed(feats, rois, V, S, O_, transform=True)
    ref_counts = gd['occ_counts'].astype(np.int64)
    print('occupied per RoI', counts, 'reference', ref_counts.tolist(), 'borderline', near_per_roi.tolist())
    assert np.all(np.abs(np.asarray(counts) - ref_counts) <= near_per_roi)
    # which cell every row of the packed result is: the decoder's own logits (what get_occ selects on)
    _, _, _, logits = dec._dense_logits(feats, rois[:, 4:7], V, S, O_)
    mine = dec._occupied(logits).cpu().numpy()
    assert int(mine.sum()) == got.size(0)
    row_of_cell = np.cumsum(mine) - 1
    ref_occ = lr > 0
    assert int(ref_occ.sum()) == gd['occ_pts'].shape[0]
    ref_row_of_cell = np.cumsum(ref_occ) - 1
    cells = np.nonzero(ref_occ & ~near)[0]
    assert mine[cells].all()
    err = np.abs(got.cpu().numpy()[row_of_cell[cells]] - gd['occ_pts'][ref_row_of_cell[cells]]).max()
    print('largest deviation from the reference points', err)
    assert err <= 2e-5


# ------------------------------------------------------------------------------------------------ the RoI head, files
@pytest.fixture(scope='module')
def model(dev):
    from objectcentricocccompletion_amd import config, dataset, heads, point_pool, roi_head  # noqa: F401
    from objectcentricocccompletion_amd.registry import DETECTORS
    torch.manual_seed(0)
    return DETECTORS.build(config.fromfile(CFG)['model']).to(dev).eval()


def _tracklet(dev):
    from objectcentricocccompletion_amd.tracklet import Tracklet
    g = torch.Generator().manual_seed(2)
    boxes = torch.cat([torch.rand(5, 3, generator=g) * 40 - 20, torch.tensor([[4.6, 2.0, 1.7]]).repeat(5, 1)
                       + torch.rand(5, 3, generator=g) * 0.2, torch.rand(5, 1, generator=g) * 6 - 3], 1)
    ts = [1553629304780200 + 100000 * i for i in range(5)]
    return Tracklet(boxes.to(dev), ts, torch.tensor([0.9, 0.8, 0.7, 0.6, 0.5], device=dev), type=1,
                    segment_name='segment-123_with_camera_labels', id='obj_7')


def _listing(root):
    return sorted(os.path.relpath(p, root) for p in glob.glob(os.path.join(root, '**', '*.bin'), recursive=True))


def test_save_occ_from_tracklet(dev, model, tmp_path, monkeypatch, capsys):
    from objectcentricocccompletion_amd import occ_export
    head = model.roi_head
    trk = _tracklet(dev)
    width = head.bbox_head.occ_ae_head.occ_decoder.roi_feature_channels
    feats = torch.randn(5, width, generator=torch.Generator().manual_seed(4)).to(dev)
    res = dict(fused_roi_feats=feats, nonempty_roi_mask=torch.tensor([True, True, True, False, True], device=dev))
    rois = head.tracklets2rois([trk])[0]
    exp = head.bbox_head.get_occ(feats, rois, transform=True)[0]
    assert sum(int(t.size(0)) for t in exp) > 0
    name = lambda i: os.path.join(trk.segment_name, str(trk.ts_list[i]), '1_obj_7.bin')

    def check(root, frames, scores):
        assert _listing(root) == sorted(name(i) for i in frames)
        for i in frames:
            a = occ_export.read_occ_bin(os.path.join(root, name(i)))
            assert a.dtype == np.float32 and a.shape == (exp[i].size(0), 4)
            assert np.array_equal(a[:, :3], exp[i].cpu().numpy())
            assert np.all(a[:, 3] == np.float32(scores[i]))

    scores = trk.scores.tolist()
    root = str(tmp_path / 'all')
    monkeypatch.setitem(head.test_cfg, 'occ_save_root', root)
    paths = head.save_occ_from_tracklet([trk], res)
    assert len(paths) == 5
    check(root, range(5), scores)
    for i in range(5):
        got = occ_export.load_frame_occ(root, trk.segment_name, trk.ts_list[i])
        assert np.array_equal(got, occ_export.read_occ_bin(os.path.join(root, name(i))))
    root = str(tmp_path / 'filtered')
    monkeypatch.setitem(head.test_cfg, 'occ_save_root', root)
    monkeypatch.setitem(head.test_cfg, 'min_evaluate_length', 2)
    monkeypatch.setitem(head.test_cfg, 'filter_empty_roi', True)
    capsys.readouterr()
    head.save_occ_from_tracklet([trk], res, gt_score=[1.0, 1.0, 0.25, 1.0, 0.75])
    assert f'empty roi 3 in {trk.segment_name} at {trk.ts_list[3]}' in capsys.readouterr().out
    check(root, [2, 4], [1.0, 1.0, 0.25, 1.0, 0.75])
    with pytest.raises(AssertionError):
        head.save_occ_from_tracklet([trk], res, gt_score=[1.0, 1.0])
    with pytest.raises(AssertionError):
        head.save_occ_from_tracklet([trk, trk], res)
    with pytest.raises(NotImplementedError, match='points_in_boxes_gpu'):
        head.save_occ_from_tracklet([trk], res, save_gt_occ=True)
    assert _listing(root) == sorted(name(i) for i in (2, 4))


def _run(cmd, timeout=600):
    p = subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out, err = p.communicate(timeout=timeout)
    assert p.returncode == 0, out[-2000:] + err[-3000:]
    return out


def test_tools_test_save_occ(dev, model, tmp_path):
    """tools/test.py --eval iou --save-occ DIR in a child process: one file per tracklet and frame, the occupancy IoU
    what the evaluation loop gives without the flag."""
    from objectcentricocccompletion_amd import config, occ_export
    from objectcentricocccompletion_amd.pipelines import collate_tracklets
    from objectcentricocccompletion_amd.registry import DATASETS
    from objectcentricocccompletion_amd.roi_head import occupancy_iou_metrics
    data, ckpt, out = str(tmp_path / 'data'), str(tmp_path / 'model.pth'), str(tmp_path / 'occ')
    _run([sys.executable, 'tools/make_synthetic_dataset.py', data, '--tracklets', '2', '--frames', '12'])
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    stdout = _run(['timeout', '-k', '10', '300', sys.executable, 'tools/test.py', CFG, ckpt, '--data-root', data,
                   '--eval', 'iou', '--save-occ', out])
    got = ast.literal_eval([l for l in stdout.strip().splitlines() if l.startswith('{')][-1])
    cfg = config.fromfile(CFG)
    j = lambda p: os.path.join(data, p)
    ds = DATASETS.build(dict(cfg['data']['test'], data_root=data, ann_file=j('tracklet_data/synth_training_gt_candidates.pkl'),
                             tracklet_proposals_file=j('tracklet_data/synth_training.pkl'), occ_anno_root=j('occ_gt'),
                             pose_file=j('poses.pkl')))
    assert 'save_occ' not in model.roi_head.test_cfg
    results, expected = [], []
    with torch.no_grad():
        for i in range(len(ds)):
            np.random.seed(i)
            torch.manual_seed(i)
            batch = collate_tracklets([ds[i]], dev)
            results.append(model(return_loss=False, **batch)[0])
            trk = batch['tracklet'][0]                                          # the tracklet the RoI head is given
            expected += [os.path.join(str(trk.segment_name), str(ts), f'{trk.type}_{trk.id}.bin') for ts in trk.ts_list]
    assert got == occupancy_iou_metrics(results)
    assert len(ds) == 2 and len(expected) == 24 and _listing(out) == sorted(expected)
    rows = 0
    for rel in expected:
        seg, ts, _ = rel.split(os.sep)
        a = occ_export.load_frame_occ(out, seg, ts)
        assert a.shape[1] == 4 and np.isfinite(a).all()
        rows += a.shape[0]
    assert rows > 0
