"""Checkpoint evaluation on the MI355X: the occupancy-count kernel (csrc/occ_iou_count.hip) against the ATen counting it
replaces, test_occ with and without it, and tools/test.py end to end -- one process against an in-process loop, two
ranks on one GPU against one rank."""
import ast
import os
import pickle
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'ococcnet_mi355x.py')


def _decoder(pos_thresh):
    from objectcentricocccompletion_amd.occ.occ_base import OccDecoder
    cfg = types.SimpleNamespace(cls_dim=1, pos_thresh=pos_thresh)
    return types.SimpleNamespace(get_cls_from_pred=lambda p: OccDecoder.get_cls_from_pred(cfg, p))


def _case(n, K, labels, seed, dev, pos_thresh=0.5):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(n, K, generator=g) * 3
    thr = float(np.log(pos_thresh / (1 - pos_thresh)))
    near = torch.tensor([thr, np.nextafter(np.float32(thr), np.float32(1)), np.nextafter(np.float32(thr), np.float32(-1)),
                         float('inf'), float('-inf'), float('nan'), 1e-7, -1e-7, 6e-8, 2e-7], dtype=torch.float32)
    pick = torch.rand(n, K, generator=g) < 0.2
    logits[pick] = near[torch.randint(0, len(near), (int(pick.sum()),), generator=g)]
    logits.view(-1)[min(5, n * K - 1)] = float('nan')          # at least one NaN in every case
    half = torch.rand(n, 3, generator=g) * 2 + 0.5
    xyz = (torch.rand(n, K, 3, generator=g) * 3 - 1.5) * half[:, None]
    edge = torch.rand(n, K, 3, generator=g) < 0.15                  # cells exactly on a face of the box
    sign = torch.where(torch.rand(n, K, 3, generator=g) < 0.5, -1.0, 1.0)
    xyz = torch.where(edge, sign * half[:, None].expand(n, K, 3), xyz)
    if labels == 'random':
        lab = (torch.rand(K, generator=g) < 0.5).long()
    else:
        lab = torch.full((K,), 1 if labels == 'ones' else 0, dtype=torch.long)
    return logits.to(dev), lab.to(dev), xyz.to(dev), half.to(dev)


def _aten(logits, lab, xyz, half, outside, pos_thresh=0.5):
    from objectcentricocccompletion_amd.roi_head import occ_iou_counts_aten
    n, K = logits.shape
    inter, union = occ_iou_counts_aten(_decoder(pos_thresh), logits.reshape(n * K, 1), lab, xyz,
                                       half if outside else None)
    return torch.stack([inter, union], 1)


@pytest.mark.parametrize('K', [1, 63, 64, 65, 4097, 64000])
@pytest.mark.parametrize('n', [1, 3, 10])
@pytest.mark.parametrize('outside', [False, True])
def test_count_kernel_equals_aten(dev, n, K, outside):
    from objectcentricocccompletion_amd.occ.occ_ops import occ_iou_count
    for li, labels in enumerate(['random', 'zeros', 'ones']):
        logits, lab, xyz, half = _case(n, K, labels, 1000 * n + K + li, dev)
        exp = _aten(logits, lab, xyz, half, outside)
        counts = torch.zeros(n + 3, 2, dtype=torch.long, device=dev)
        occ_iou_count(logits.reshape(n * K, 1), lab, counts, 2, 0.5, xyz if outside else None, half if outside else None)
        assert torch.equal(counts[2:2 + n], exp), (labels, counts[2:2 + n].tolist(), exp.tolist())
        assert not bool(counts[:2].any()) and not bool(counts[2 + n:].any())


def test_count_kernel_other_threshold_and_chunks_at_offsets(dev):
    """pos_thresh 0.3 with logits at and beside logit(0.3); two chunks adding into one buffer at their row offsets, and
    a chunk counted twice adds up."""
    from objectcentricocccompletion_amd.occ.occ_ops import occ_iou_count
    K = 5000
    a = _case(3, K, 'random', 7, dev, pos_thresh=0.3)
    b = _case(2, K, 'random', 8, dev, pos_thresh=0.3)
    b = (b[0], a[1], b[2], b[3])                                        # one label vector per tracklet
    counts = torch.zeros(5, 2, dtype=torch.long, device=dev)
    occ_iou_count(a[0], a[1], counts, 0, 0.3, a[2], a[3])
    occ_iou_count(b[0], b[1], counts, 3, 0.3, b[2], b[3])
    exp = torch.cat([_aten(*a, True, 0.3), _aten(*b, True, 0.3)])
    assert torch.equal(counts, exp)
    occ_iou_count(b[0], b[1], counts, 3, 0.3, b[2], b[3])
    assert torch.equal(counts[3:], 2 * exp[3:]) and torch.equal(counts[:3], exp[:3])
    from objectcentricocccompletion_amd._lib import OcoccError
    with pytest.raises(OcoccError, match='outside the count buffer'):
        occ_iou_count(b[0], b[1], counts, 4, 0.3, b[2], b[3])


# ---------------------------------------------------------------------------------------------- the model on files
def _run(cmd, env=None, timeout=900):
    p = subprocess.Popen(cmd, cwd=ROOT, env=env or dict(os.environ), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True)
    out, err = p.communicate(timeout=timeout)
    assert p.returncode == 0, out[-2000:] + err[-3000:]
    return out


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    """5 synthetic tracklets of 40 frames and a checkpoint of tools/train.py after 2 iterations."""
    root = tmp_path_factory.mktemp('eval')
    data, work = str(root / 'data'), str(root / 'work')
    _run([sys.executable, 'tools/make_synthetic_dataset.py', data, '--tracklets', '5', '--frames', '40'], timeout=300)
    _run([sys.executable, 'tools/train.py', CFG, '--data-root', data, '--iters', '2', '--work-dir', work])
    return types.SimpleNamespace(root=root, data=data, ckpt=os.path.join(work, 'latest.pth'))


def _model_and_data(tree, dev):
    from objectcentricocccompletion_amd import config, dataset, heads, point_pool, roi_head  # noqa: F401
    from objectcentricocccompletion_amd.registry import DATASETS, DETECTORS
    cfg = config.fromfile(CFG)
    j = lambda p: os.path.join(tree.data, p)
    ds_cfg = dict(cfg['data']['test'], data_root=tree.data, ann_file=j('tracklet_data/synth_training_gt_candidates.pkl'),
                  tracklet_proposals_file=j('tracklet_data/synth_training.pkl'), occ_anno_root=j('occ_gt'),
                  pose_file=j('poses.pkl'))
    ds = DATASETS.build(ds_cfg)
    model = DETECTORS.build(cfg['model']).to(dev)
    model.load_state_dict(torch.load(tree.ckpt, map_location=dev)['state_dict'])
    return model.eval(), ds


def _loop(model, ds, dev, seed=0):
    """the hand-written evaluation: model(return_loss=False) per tracklet, each tracklet's pipeline seeded with seed + i"""
    from objectcentricocccompletion_amd.pipelines import collate_tracklets
    out = []
    with torch.no_grad():
        for i in range(len(ds)):
            np.random.seed(seed + i)
            torch.manual_seed(seed + i)
            out.append(model(return_loss=False, **collate_tracklets([ds[i]], dev))[0])
    return out


def _metrics_line(stdout):
    return ast.literal_eval([l for l in stdout.strip().splitlines() if l.startswith('{')][-1])


def test_test_occ_kernel_equals_aten_counting(dev, tree, monkeypatch):
    from objectcentricocccompletion_amd import roi_head
    model, ds = _model_and_data(tree, dev)
    tcfg = model.roi_head.test_cfg
    for outside, chunk in ((True, 10), (False, 7)):
        monkeypatch.setitem(tcfg, 'ignore_outside_occ', outside)
        monkeypatch.setitem(tcfg, 'iou_chunk_size', chunk)
        runs = []
        for kernel in (True, False):
            monkeypatch.setattr(roi_head, 'OCC_IOU_KERNEL', kernel)
            runs.append(_loop(model, ds, dev))
        counted = 0
        for a, b in zip(*runs):
            assert len(a['inters']) == len(b['inters']) and len(a['gt_boxes']) == len(b['gt_boxes'])
            for key in ('inters', 'unions', 'gt_boxes'):
                for x, y in zip(a[key], b[key]):
                    assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), key
            counted += sum(int(x.numel()) for x in a['inters'])
        assert counted >= 5 * 30                                        # every tracklet has matched, counted RoIs
        assert roi_head.occupancy_iou_metrics(runs[0]) == roi_head.occupancy_iou_metrics(runs[1])


def test_tools_test_equals_in_process_loop(dev, tree):
    from objectcentricocccompletion_amd.roi_head import occupancy_iou_metrics
    out_pkl = str(tree.root / 'r.pkl')
    stdout = _run(['timeout', '-k', '10', '900', sys.executable, 'tools/test.py', CFG, tree.ckpt, '--data-root', tree.data,
                   '--eval', 'iou', '--out', out_pkl])
    got = _metrics_line(stdout)
    model, ds = _model_and_data(tree, dev)
    exp_results = _loop(model, ds, dev)
    exp = occupancy_iou_metrics(exp_results)
    assert set(exp) >= {'iou', 'miou_track', 'miou_box'} and got == exp
    with open(out_pkl, 'rb') as f:
        res = pickle.load(f)
    assert len(res) == len(ds) == 5
    for i, (r, e) in enumerate(zip(res, exp_results)):
        assert r['out_tracklets'][0].id == ds.get_data_info(i)['tracklet'].id       # dataset order
        for key in ('inters', 'unions'):
            assert len(r[key]) == len(e[key]) and all(torch.equal(x, y) for x, y in zip(r[key], e[key]))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_on_one_gpu_equal_one_rank(dev, tree):
    """gloo, both ranks on cuda:0, the SIR layers one launch per block (OCOCC_SIR_FUSED=0: the one-launch layer assumes
    one process per device); 5 tracklets = shards of 3 + 2."""
    base = dict(os.environ, OCOCC_SIR_FUSED='0')
    cmd = [sys.executable, 'tools/test.py', CFG, tree.ckpt, '--data-root', tree.data, '--eval', 'iou']
    one_pkl, two_pkl = str(tree.root / 'one.pkl'), str(tree.root / 'two.pkl')
    one = _metrics_line(_run(cmd + ['--out', one_pkl], env=base))
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(base, RANK=str(r), LOCAL_RANK='0', WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        procs.append(subprocess.Popen(cmd + ['--out', two_pkl, '--launcher', 'pytorch', '--dist-backend', 'gloo',
                                             '--tmpdir', str(tree.root / 'parts')],
                                      cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=900))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, o[-2000:] + e[-3000:]
    assert _metrics_line(outs[0][0]) == one
    assert not [l for l in outs[1][0].splitlines() if l.startswith('{')]        # only rank 0 prints the metrics
    with open(one_pkl, 'rb') as f:
        a = pickle.load(f)
    with open(two_pkl, 'rb') as f:
        b = pickle.load(f)
    assert len(a) == len(b) == 5
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y)
        tx, ty = x['out_tracklets'][0], y['out_tracklets'][0]
        assert tx.id == ty.id and tx.ts_list == ty.ts_list
        # (refined boxes and scores: f32 results of a forward pass whose scatter means add with float atomics, so two
        # runs agree to rounding, not bit for bit; the integer counts below are exact)
        assert torch.allclose(tx.boxes, ty.boxes, rtol=1e-5, atol=1e-5), float((tx.boxes - ty.boxes).abs().max())
        assert torch.allclose(tx.scores, ty.scores, rtol=1e-5, atol=1e-6)
        for key in ('inters', 'unions', 'gt_boxes'):
            assert len(x[key]) == len(y[key]) and all(torch.equal(u, v) for u, v in zip(x[key], y[key]))
