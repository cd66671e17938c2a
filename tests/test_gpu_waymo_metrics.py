"""GPU suite: the matching kernels of the native Waymo detection metric (csrc/frame_match.hip, waymo_metrics.py) against
the float64 checker tests/waymo_metrics_ref.py -- overlaps to 5e-5 absolute, match indices exactly on frames generated so
that float32 against float64 cannot flip a decision, ties by the file-order rules, byte-identical repeats, the whole
metric to 1e-12, and tools/test.py / tools/waymo_detection_metrics.py end to end on the synthetic tree.

Overlap tolerance 5e-5: a CPU emulation of float32 Sutherland-Hodgman clipping in the box-local frame differed from the
hull checker by at most 7.0e-6 over 4 000 vehicle-like pairs at +-75 m (float32 rounding of the inputs included); the
margin of about 7x covers sinf / cosf and contraction differences of the real kernel."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import waymo_metrics_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'ococcnet_mi355x.py')
IOU_TOL = 5e-5


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _pair_ious(pd_boxes, gt_boxes):
    """IoU of pd_boxes[i] with gt_boxes[i] through the kernels: every pair is a frame of its own (1 x 1, type 1, threshold
    as low as the export takes), so match_iou is the pair's IoU wherever it is above that threshold"""
    from objectcentricocccompletion_amd import waymo_metrics as M
    dev = _dev()
    n = len(pd_boxes)
    ones = torch.ones(n, dtype=torch.int32, device=dev)
    off = list(range(n + 1))
    up = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32).reshape(n, 7)).to(dev)
    mg, mi = M.frame_match(up(pd_boxes), ones, ones, off, up(gt_boxes), ones, ones, off, iou_thresholds=(0, 1e-30, .5, .5, .5))
    return mg.cpu().numpy(), mi.cpu().numpy().astype(np.float64)


def _rand_box(rng, extent=75.0):
    return [rng.uniform(-extent, extent), rng.uniform(-extent, extent), rng.uniform(-1, 2), rng.uniform(3.5, 6.0),
            rng.uniform(1.6, 2.4), rng.uniform(1.4, 2.2), rng.uniform(-math.pi, math.pi)]


def _perturbed(rng, g):
    s = float(rng.choice([0.02, 0.1, 0.3]))
    p = list(g)
    p[0] += rng.normal(0, s) * 3
    p[1] += rng.normal(0, s) * 3
    p[2] += rng.normal(0, s)
    for k in (3, 4, 5):
        p[k] *= 1 + rng.normal(0, s / 2)
    p[6] += rng.normal(0, s / 2)
    return p


def test_overlap_against_the_checker():
    rng = np.random.default_rng(0)
    cases = {}
    g = [_rand_box(rng) for _ in range(3000)]
    cases['random pairs at +-75 m'] = ([_perturbed(rng, b) for b in g], g)
    g = [_rand_box(rng) for _ in range(500)]
    p = [_perturbed(rng, b) for b in g]
    for a, b in zip(p, g):
        a[6] = b[6]
    cases['equal yaw'] = (p, g)
    g = [_rand_box(rng) for _ in range(200)]
    cases['identical boxes'] = ([list(b) for b in g], g)
    g = [[rng.uniform(-75, 75), rng.uniform(-75, 75), 0.0, rng.uniform(4, 12), rng.uniform(0.02, 0.1), 1.5,
          rng.uniform(-math.pi, math.pi)] for _ in range(500)]
    cases['thin boxes'] = ([[b[0] + rng.normal(0, 0.02), b[1] + rng.normal(0, 0.02), 0.1, b[3], b[4], b[5], b[6] + rng.normal(0, 0.005)]
                            for b in g], g)
    g = [_rand_box(rng) for _ in range(300)]
    cases['one box inside the other'] = ([[b[0], b[1], b[2], b[3] * 0.4, b[4] * 0.4, b[5] * 0.5, b[6] + rng.uniform(-3, 3)] for b in g], g)
    f32 = lambda boxes: [[float(np.float32(v)) for v in b] for b in boxes]
    worst = 0.0
    for name, (p, g) in cases.items():
        p, g = f32(p), f32(g)
        mg, got = _pair_ious(p, g)
        exp = np.array([R.iou3d(a, b) for a, b in zip(p, g)])
        err = np.abs(got - exp)
        print(f'{name}: {len(p)} pairs, {int((exp > 0).sum())} overlapping, worst |IoU difference| {err.max():.3e}')
        worst = max(worst, err.max())
        assert ((mg == np.arange(len(p))) == (got > 0)).all()
        assert err.max() <= IOU_TOL, name
        if name == 'identical boxes':
            assert np.abs(got - 1).max() <= IOU_TOL
        if name != 'thin boxes':
            assert (exp > 0.05).mean() > 0.5, 'the case does not exercise the clip'
    print(f'worst over all cases {worst:.3e}')


def test_degenerate_boxes_give_zero_and_never_match():
    base = [70.0, -70.0, 1.0, 4.5, 2.0, 1.6, 0.3]
    bad = []
    for k in (3, 4, 5):
        for v in (0.0, -1.0, float('nan'), float('inf')):
            b = list(base)
            b[k] = v
            bad.append(b)
    for k in (0, 1, 2, 6):
        for v in (float('nan'), float('inf')):
            b = list(base)
            b[k] = v
            bad.append(b)
    n = len(bad)
    mg, mi = _pair_ious(bad + [base] * n + [base], [base] * n + bad + [base])
    assert (mg[:-1] == -1).all() and (mi[:-1] == 0).all()
    assert mg[-1] == 2 * n and abs(mi[-1] - 1) <= IOU_TOL       # (the control: the same call matches a sound pair)
    assert all(R.iou3d(a, base) == 0.0 for a in bad)


def _run_match(preds, gts, assume_points=False, **kw):
    """preds / gts (dicts) through pack + frame_match -> per prediction (file order) the ground-truth file index or -1,
    and the raw device outputs"""
    from objectcentricocccompletion_amd import waymo_metrics as M
    dev = _dev()
    pk = M.pack(M.columns(preds), M.columns(gts), assume_points)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(dev)
    mg, mi = M.frame_match(up(pk['pd_boxes'], np.float32), up(pk['pd_type'], np.int32), up(pk['pd_eligible'], np.int32),
                           pk['pd_offsets'], up(pk['gt_boxes'], np.float32), up(pk['gt_type'], np.int32),
                           up(pk['gt_eligible'], np.int32), pk['gt_offsets'], **kw)
    packed = mg.cpu().numpy()
    out = np.full(len(preds), -1, dtype=np.int64)
    out[pk['pd_order']] = np.where(packed >= 0, pk['gt_order'][np.maximum(packed, 0)], -1) if len(gts) else -1
    return out.tolist(), mg, mi


@pytest.mark.parametrize('name,sizes', [
    ('no predictions', [(0, 7)]), ('no ground truth', [(9, 0)]), ('one by one', [(1, 1)] * 3), ('typical', [(80, 60)] * 4),
    ('more than a wave, more than LDS holds', [(600, 400)]), ('mixed with empty frames', [(0, 0), (5, 3), (0, 4), (7, 0), (80, 60), (1, 1)]),
])
def test_matching_is_exact(name, sizes):
    rng = np.random.default_rng(len(name))
    preds, gts, drawn, redrawn = R.decisive_frames(rng, sizes)
    assert redrawn <= 0.05 * drawn
    exp = R.match(preds, gts)
    got, mg, mi = _run_match(preds, gts)
    assert got == exp
    assert ((mi > 0) == (mg >= 0)).all()
    if sizes[0] in ((80, 60), (600, 400)):
        assert sum(m >= 0 for m in exp) > 100         # the case matches something


def test_matching_is_exact_on_5000_frames_in_one_call_and_in_chunks():
    rng = np.random.default_rng(7)
    sizes = [(int(rng.integers(0, 13)), int(rng.integers(0, 11))) for _ in range(5000)]
    preds, gts, drawn, redrawn = R.decisive_frames(rng, sizes, types=(1, 2))
    print(f'{drawn} frames drawn, {redrawn} redrawn ({100.0 * redrawn / drawn:.2f} %)')
    assert redrawn <= 0.05 * drawn
    exp = R.match(preds, gts)
    got, mg, mi = _run_match(preds, gts)
    assert got == exp
    assert sum(m >= 0 for m in exp) > 5000
    # the same input cut into many workspace chunks: the same bytes
    _, mg2, mi2 = _run_match(preds, gts, workspace_budget=64 << 10)
    assert torch.equal(mg, mg2) and torch.equal(mi.view(torch.int32), mi2.view(torch.int32))


def test_ties_go_by_file_order():
    """equal scores: the earlier prediction in the file chooses first; equal IoU (duplicated ground truth): the lower
    file index is taken"""
    box = [60.0, -50.0, 1.0, 4.5, 2.0, 1.6, 0.4]
    near = [60.1, -50.0, 1.0, 4.5, 2.0, 1.6, 0.4]
    mk = R.make_object
    gts = [mk([0, 0, 0, 4, 2, 1.5, 0], 1, points=9), mk(box, 1, points=9), mk(box, 1, points=9), mk(box, 1, points=9)]
    preds = [mk(near, 1, 0.5), mk(near, 1, 0.5), mk(box, 1, 0.5), mk(near, 1, 0.5), mk(near, 1, 0.7)]
    exp = R.match(preds, gts)
    assert exp == [2, 3, -1, -1, 1]        # 0.7 first -> index 1; then the 0.5s in file order -> 2, 3; nothing is left
    got, _, mi = _run_match(preds, gts)
    assert got == exp
    # one prediction, two identical candidates: the lower index
    assert _run_match([mk(near, 1, 0.9)], [mk(box, 1, points=9), mk(box, 1, points=9)])[0] == [0]
    # an ignored duplicate in front is skipped, a LEVEL_2 one is not
    assert _run_match([mk(near, 1, 0.9)], [mk(box, 1, points=0), mk(box, 1, points=3), mk(box, 1, points=9)])[0] == [1]
    assert _run_match([mk(near, 1, 0.9)], [mk(box, 1, points=0), mk(box, 1, points=9)], assume_points=True)[0] == [0]
    # another type never competes
    assert _run_match([mk(near, 2, 0.9)], [mk(box, 1, points=9)])[0] == [-1]


def test_two_calls_give_identical_bytes():
    rng = np.random.default_rng(21)
    preds, gts = [], []
    for f in range(60):
        p, g = R.random_frame(rng, 80, 60, ts=f)
        preds += p
        gts += g
    _, mg1, mi1 = _run_match(preds, gts)
    _, mg2, mi2 = _run_match(preds, gts)
    assert (mg1 >= 0).sum().item() > 1000
    assert torch.equal(mg1, mg2) and torch.equal(mi1.view(torch.int32), mi2.view(torch.int32))


def _mixed_scene(rng):
    sizes = [(int(rng.integers(5, 60)), int(rng.integers(5, 50))) for _ in range(30)]
    preds, gts, drawn, redrawn = [], [], 0, 0
    for s, part in enumerate((sizes[:15], sizes[15:])):
        p, g, d, r = R.decisive_frames(rng, part, ctx=f'segment-{s}', ts0=1000 * s)
        preds, gts, drawn, redrawn = preds + p, gts + g, drawn + d, redrawn + r
    assert redrawn <= 0.05 * drawn
    preds = [preds[i] for i in rng.permutation(len(preds))]
    gts = [gts[i] for i in rng.permutation(len(gts))]
    return preds, gts


def test_whole_metric_equals_the_checker():
    from objectcentricocccompletion_amd import waymo_io as W
    from objectcentricocccompletion_amd import waymo_metrics as M
    preds, gts = _mixed_scene(np.random.default_rng(3))
    assert {R.gt_level(g) for g in gts} == {0, 1, 2} and any(p['overlap_with_nlz'] for p in preds)
    assert {R._range_bin(g) for g in gts} == {0, 1, 2} and {g['type'] for g in gts} == {1, 2, 3, 4}
    tab, exp = R.detection_metrics(preds, gts)
    text, got = M.detection_metrics(preds, gts)
    assert got == W.parse_detection_metrics(text) and set(got) == set(exp)
    worst = max(abs(got[k] - exp[k]) for k in exp)
    print(f'largest |ap_dict difference| {worst:.3e}; Vehicle/L1 mAP {exp["Vehicle/L1 mAP"]:.6f}')
    assert worst <= 1e-12
    assert min(exp[f'{c}/L{l} mAP'] for c in ('Vehicle', 'Pedestrian', 'Sign', 'Cyclist') for l in (1, 2)) > 0.01
    lines = {l.split(':')[0]: l for l in text.splitlines() if not l.startswith('#')}
    assert list(lines) == list(tab)
    for k, (a, h) in tab.items():
        assert float(lines[k].split('mAP ')[1].split(']')[0]) == pytest.approx(a, abs=1e-12), k
        assert float(lines[k].split('mAPH ')[1].split(']')[0]) == pytest.approx(h, abs=1e-12), k
    assert sum(1 for k, v in tab.items() if k.startswith('RANGE') and v[0] > 0) >= 20
    # files whose ground truth has no point counts: everything ignored, unless assume_points
    bare = [dict(g, num_lidar_points_in_box=0, detection_difficulty_level=0) for g in gts]
    assert max(M.detection_metrics(preds, bare)[1].values()) == 0.0
    _, got = M.detection_metrics(preds, bare, assume_points=True)
    _, exp = R.detection_metrics(preds, bare, assume_points=True)
    assert max(abs(got[k] - exp[k]) for k in exp) <= 1e-12 and got['Vehicle/L1 mAP'] > 0.01


def _run(cmd, timeout=900, env=None):
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p.stdout


def _dict_line(stdout):
    import ast
    return ast.literal_eval([l for l in stdout.splitlines() if l.startswith('{')][-1])


def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _same(a, b, tol):
    from objectcentricocccompletion_amd import waymo_io as W
    return all(abs(a[k] - b[k]) <= tol for k in W.AP_KEYS)


def test_end_to_end_on_the_synthetic_tree(tmp_path):
    """Separate runs of the model agree to rounding only (its scatter means add with float atomics, tests/test_gpu_eval.py),
    so the refined boxes of two runs differ in their last bits: AP is a step function of the matches and APH moves with
    the headings by as much, hence 1e-6 between RUNS; on the same result file the two routes must agree exactly."""
    from objectcentricocccompletion_amd import waymo_io as W
    data, work = str(tmp_path / 'data'), str(tmp_path / 'work')
    env = dict(os.environ, OCOCC_SIR_FUSED='0')      # (two processes on one device: the per-block SIR launches)
    _run([sys.executable, 'tools/make_synthetic_dataset.py', data, '--tracklets', '5', '--frames', '40'], 300)
    _run([sys.executable, 'tools/train.py', CFG, '--data-root', data, '--iters', '2', '--work-dir', work])
    ckpt = os.path.join(work, 'latest.pth')
    base = [sys.executable, 'tools/test.py', CFG, ckpt, '--data-root', data]
    native = ['--eval', 'iou', 'waymo_native', '--eval-options']
    one = _dict_line(_run(base + native + [f'pklfile_prefix={tmp_path}/one'], env=env))
    assert 'iou' in one and set(W.AP_KEYS) <= set(one) and all(0.0 <= one[k] <= 1.0 for k in W.AP_KEYS)
    text = open(f'{tmp_path}/one.txt').read()
    assert os.path.isfile(f'{tmp_path}/one.bin') and 'OBJECT_TYPE_TYPE_VEHICLE_LEVEL_1' in text
    assert W.parse_detection_metrics(text) == {k: one[k] for k in W.parse_detection_metrics(text)}
    gt = os.path.join(data, 'waymo_format', 'gt.bin')
    tool = os.path.join(ROOT, 'tools', 'waymo_detection_metrics.py')
    # the stand-alone tool on the file that run wrote: exactly the same numbers
    assert W.parse_detection_metrics(_run([tool, f'{tmp_path}/one.bin', gt])) == W.parse_detection_metrics(text)
    # ... and in place of the Waymo binary, through the unchanged waymo_io.evaluate subprocess path (a fresh child process)
    via = _dict_line(_run(base + ['--eval', 'waymo', '--eval-options', f'pklfile_prefix={tmp_path}/via',
                                  f'metrics_main={tool}'], env=env))
    assert _same(via, one, 1e-6), (via, one)
    assert W.parse_detection_metrics(open(f'{tmp_path}/via.txt').read()) == {k: via[k] for k in via}
    # two ranks on one GPU
    port, procs, outs = _free_port(), [], []
    for r in range(2):
        e = dict(env, RANK=str(r), LOCAL_RANK='0', WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        procs.append(subprocess.Popen(base + ['--launcher', 'pytorch', '--dist-backend', 'gloo', '--tmpdir', f'{tmp_path}/parts'] +
                                      native + [f'pklfile_prefix={tmp_path}/two'], cwd=ROOT, env=e, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
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
    two = _dict_line(outs[0][0])
    assert _same(two, one, 1e-6), (two, one)
    assert len(W.read_bin(f'{tmp_path}/two.bin')) == len(W.read_bin(f'{tmp_path}/one.bin')) > 0
    # perfect predictions: the ground truth scored against itself.  Every object counts with --assume-points (the 0-point
    # objects become LEVEL_1): 1.0 throughout.
    out = _run([tool, gt, gt, '--assume-points'])
    ap = W.parse_detection_metrics(out)
    for k in ('Vehicle/L1 mAP', 'Vehicle/L1 mAPH', 'Vehicle/L2 mAP', 'Vehicle/L2 mAPH'):
        assert ap[k] == pytest.approx(1.0, abs=1e-12), k
    assert ap['Pedestrian/L1 mAP'] == 0.0
    assert 'Hungarian' in out and 'recall-delta' in out
    # Without it the file's 0-point objects are ignored, so the "predictions" on them are false positives, all at score 1:
    # per 10 frames of an object 1 ignored, 2 LEVEL_2 (frames 5 and 7), 7 LEVEL_1 -> LEVEL_2 precision 9/10 at recall 1,
    # LEVEL_1 (matches to LEVEL_2 objects left out) 7/8.
    ap = W.parse_detection_metrics(_run([tool, gt, gt]))
    assert ap['Vehicle/L1 mAP'] == pytest.approx(7 / 8, abs=1e-12) and ap['Vehicle/L2 mAP'] == pytest.approx(9 / 10, abs=1e-12)
    assert ap['Vehicle/L1 mAPH'] == pytest.approx(7 / 8, abs=1e-12)
