"""Tracklet data preparation on the MI355X (csrc/tracklet_crop.hip, csrc/tracklet_iou.hip,
objectcentricocccompletion_amd/ctrl_prep.py, tools/ctrl/*).  Fixtures are built here from fixed seeds; the checkers are
numpy float64 restatements, the parent's own one-to-one IoU kernel and the C oracle (oracle.oracle.aligned_iou3d).

Measured on an MI355X with this file's seeds (profiles/ctrl_prep.md):
  crop: the 1e-3 m shell holds 67 of 211 873 points, 0.0316 % (cap 1 %);
  max IoU: the parent's kernel deviates from the oracle by at most 1.568e-5 on the 1 741 common-frame pairs of this fixture
  (boxes out to 75 m), ococc_tracklet_max_iou_f32 by the same 1.568e-5 (held to twice the parent's figure, computed
  at run time); candidates at 0.5: no pair of the fixture lies within that distance of the threshold (cap 1 %)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = 'configs/ococcnet_mi355x.py'


# ---------------------------------------------------------------------------------------------- crop
def in_box_f64(xyz, box):
    """check_pt_in_box3d (points_in_boxes_cuda.cu:24-49) in float64"""
    xyz, box = np.asarray(xyz, np.float64), np.asarray(box, np.float64)
    x, y, zb, w, l, h, yaw = box[:7]
    rot = yaw + np.pi / 2
    dx, dy = xyz[:, 0] - x, xyz[:, 1] - y
    lx = dx * np.cos(rot) - dy * np.sin(rot)
    ly = dx * np.sin(rot) + dy * np.cos(rot)
    return (np.abs(xyz[:, 2] - (zb + h / 2)) <= h / 2) & (lx > -l / 2) & (lx < l / 2) & (ly > -w / 2) & (ly < w / 2)


def grown(box, e):
    """the box with every face moved outwards by e (inwards for e < 0)"""
    b = np.asarray(box, np.float64).copy()
    b[3:6] += 2 * e
    b[2] -= e
    return b


def in_shell(xyz, box, e=1e-3):
    return in_box_f64(xyz, grown(box, e)) & ~in_box_f64(xyz, grown(box, -e))


def crop_scene(seed=11):
    """6 frames of unequal size (one empty, one without boxes, the largest 120 000 points), per frame up to 14 boxes
    enlarged by 1 m within 75 m of the origin, yaw over the whole circle, some nearly on top of each other, one high
    above every point; half of the points scattered around the boxes, half over the whole range."""
    rng = np.random.default_rng(seed)
    sizes = [120_000, 0, 30_000, 50_000, 7_777, 4_096]
    num_boxes = [14, 5, 9, 0, 12, 3]
    points, boxes = [], []
    for n, nb in zip(sizes, num_boxes):
        r, a = rng.uniform(5, 75, nb), rng.uniform(-np.pi, np.pi, nb)
        bx = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-1.5, 0.5, nb), rng.uniform(1.6, 2.4, nb) + 2,
                       rng.uniform(3.8, 5.5, nb) + 2, rng.uniform(1.4, 2.0, nb) + 2, rng.uniform(-np.pi, np.pi, nb)], 1)
        if nb >= 4:
            bx[1, :3] = bx[0, :3] + [0.8, -0.5, 0.1]     # overlapping enlarged boxes
            bx[3, :3] = bx[2, :3] + [1.5, 1.0, 0.0]
            bx[nb - 1, 2] = 40.0                          # no point up there
        half = n // 2
        far = rng.uniform([-80, -80, -3], [80, 80, 5], (n - half, 3))
        if nb:
            own = rng.integers(0, nb, half)
            near = bx[own, :3] + [0, 0, 1.5] + rng.normal(0, [3.0, 3.0, 1.5], (half, 3))
            near[bx[own, 2] > 10] = rng.uniform([-80, -80, -3], [80, 80, 5], (int((bx[own, 2] > 10).sum()), 3))
        else:
            near = rng.uniform([-80, -80, -3], [80, 80, 5], (half, 3))
        xyz = np.concatenate([near, far], 0)[rng.permutation(n)] if n else np.zeros((0, 3))
        points.append(np.concatenate([xyz, rng.random((n, 3))], 1).astype(np.float32))
        boxes.append(bx.astype(np.float32))
    return points, boxes


def expected_crop(points, boxes):
    return [np.nonzero(in_box_f64(p[:, :3], b))[0] for p, bx in zip(points, boxes) for b in bx]


def run_crop(points, boxes, dev):
    from objectcentricocccompletion_amd import ctrl_prep as cp
    counts, lists = cp.crop_frames([torch.from_numpy(p).to(dev) for p in points], [torch.from_numpy(b).to(dev) for b in boxes])
    return counts.numpy(), [i.cpu().numpy() for i in lists]


def test_crop_exact_outside_the_rounding_shell(dev):
    points, boxes = crop_scene()
    total = sum(len(p) for p in points)
    kept = []
    for p, bx in zip(points, boxes):
        shell = np.zeros(len(p), bool)
        for b in bx:
            shell |= in_shell(p[:, :3], b)
        kept.append(np.ascontiguousarray(p[~shell]))
    removed = total - sum(len(p) for p in kept)
    print(f'crop: {removed} of {total} points in the 1e-3 m shell ({100 * removed / total:.4f} %)')
    assert removed <= 0.01 * total
    assert max(len(p) for p in kept) >= 100_000
    exp = expected_crop(kept, boxes)
    counts, lists = run_crop(kept, boxes, dev)
    assert counts.dtype == np.int64 and counts.tolist() == [len(e) for e in exp]
    assert len(lists) == len(exp) == 43
    for got, e in zip(lists, exp):
        assert np.array_equal(got, e)
    assert min(counts) == 0 and max(counts) > 1000
    members = np.zeros(len(kept[0]), np.int32)          # a point may be in several boxes
    for e in exp[:14]:
        members[e] += 1
    assert members.max() >= 2


def test_crop_counts_within_shell_population(dev):
    points, boxes = crop_scene()
    exp = expected_crop(points, boxes)
    shell = [int(in_shell(p[:, :3], b).sum()) for p, bx in zip(points, boxes) for b in bx]
    counts, lists = run_crop(points, boxes, dev)
    worst = max(abs(int(c) - len(e)) for c, e in zip(counts, exp))
    print(f'crop, nothing removed: largest count difference {worst}, shell populations up to {max(shell)}')
    for c, e, s, got in zip(counts, exp, shell, lists):
        assert abs(int(c) - len(e)) <= s and len(got) == c and (np.diff(got) > 0).all()


# ---------------------------------------------------------------------------------------------- max IoU, candidates
def iou_scene(seed=5, P=64, G=40, T=160, reach=75.0):
    """One segment of T frames.  G GT tracks with gaps (a few of a single frame, a few confined to the first quarter);
    P predictions: a jittered copy of every GT track (offset growing with the track index: IoU from ~0.95 down to ~0.2),
    one exact copy, single-frame predictions, predictions with no GT nearby, predictions confined to the last quarter
    (no frame in common with the early GT tracks)."""
    from objectcentricocccompletion_amd.tracklet import Tracklet
    rng = np.random.default_rng(seed)
    stamps = [1_000_000 + 100_000 * f for f in range(T)]

    def track(frames, start=None):
        r, a = rng.uniform(5, reach - 8), rng.uniform(-np.pi, np.pi)
        c = np.array([r * np.cos(a), r * np.sin(a)]) if start is None else start
        v, yaw0 = rng.normal(0, 0.04, 2), rng.uniform(-np.pi, np.pi)
        size = [rng.uniform(1.7, 2.3), rng.uniform(4.0, 5.4), rng.uniform(1.4, 1.9)]
        f = np.asarray(frames, np.float64)[:, None]
        xy = c + v * (f - f[0])
        return np.concatenate([xy, np.full_like(f, rng.uniform(-1, 0.5)), np.tile(size, (len(f), 1)), yaw0 + 0.003 * (f - f[0])], 1)

    def mk(boxes, frames, name):
        return Tracklet(torch.from_numpy(boxes.astype(np.float32)), [stamps[f] for f in frames], None, 0, 'segment-000', name)

    gts, pds = [], []
    for g in range(G):
        if g < 4:
            frames = [int(rng.integers(0, T))]                                     # a single frame
        elif g < 10:
            frames = sorted(rng.choice(T // 4, int(rng.integers(10, T // 4)), replace=False).tolist())   # early only
        else:
            lo = int(rng.integers(0, T - 40))
            span = np.arange(lo, min(T, lo + int(rng.integers(30, 140))))
            frames = span[rng.random(len(span)) > 0.12].tolist()                   # gaps
        gts.append(mk(track(frames), frames, f'gt{g:02d}'))
    sigma = np.linspace(0.02, 0.55, G)
    for g, t in enumerate(gts):                                                     # jittered copies
        keep = np.nonzero(rng.random(len(t)) > 0.1)[0] if len(t) > 1 else np.arange(1)
        b = t.boxes.numpy()[keep].astype(np.float64)
        ang = rng.uniform(-np.pi, np.pi)                     # a constant offset per track (the maximum over the frames
        b[:, :2] += 2.2 * sigma[g] * np.array([np.cos(ang), np.sin(ang)])   # would undo independent per-frame jitter)
        b += rng.normal(0, 1, b.shape) * 0.03 * [1, 1, 0.3, 0.3, 0.3, 0.3, 0.15]
        frames = [stamps.index(t.ts_list[k]) for k in keep]
        pds.append(mk(b, frames, f'pd{g:02d}'))
    pds.append(mk(gts[20].boxes.numpy().astype(np.float64), [stamps.index(s) for s in gts[20].ts_list], 'pd_same'))
    while len(pds) < P - 8:                                                         # nothing nearby
        frames = np.arange(0, T, 2).tolist()
        pds.append(mk(track(frames, start=np.array([0.0, 0.0]) + rng.uniform(-2, 2, 2)) + [0, 0, 30, 0, 0, 0, 0], frames, f'pd_far{len(pds)}'))
    while len(pds) < P:                                                             # late only
        frames = np.arange(3 * T // 4 + len(pds) % 3, T).tolist()
        pds.append(mk(track(frames), frames, f'pd_late{len(pds)}'))
    return pds, gts


def pairwise(pds, gts, fn):
    """[P, G] of fn(pd boxes, gt boxes at the common timestamps) -> float, 0 without a common timestamp; and the mask"""
    out = np.zeros((len(pds), len(gts)), np.float32)
    common = np.zeros(out.shape, bool)
    for i, p in enumerate(pds):
        for j, g in enumerate(gts):
            i1, i2 = p.common_frames(g)
            if i1:
                common[i, j] = True
                out[i, j] = fn(p, g, i1, i2)
    return out, common


@pytest.fixture(scope='module')
def iou_case(dev):
    from objectcentricocccompletion_amd import ctrl_prep as cp
    pds, gts = iou_scene()
    on = lambda trks: [type(t)(t.boxes.to(dev), t.ts_list, None, 0, t.segment_name, t.id) for t in trks]
    dp, dg = on(pds), on(gts)
    parent, common = pairwise(dp, dg, lambda p, g, i1, i2: float(p.intersection_ious(g).max()))
    oracle, _ = pairwise(pds, gts, lambda p, g, i1, i2: float(O.aligned_iou3d(p.boxes.numpy()[i1], g.boxes.numpy()[i2]).max()))
    got = cp.tracklet_max_iou(dp, dg).cpu().numpy()
    return dict(pds=pds, gts=gts, parent=parent, oracle=oracle, common=common, got=got)


def test_max_iou_equals_parent_kernel_and_oracle(iou_case):
    c = iou_case
    P, G = c['got'].shape
    assert P >= 64 and G >= 32 and c['got'].dtype == np.float32
    lens_p, lens_g = [len(t) for t in c['pds']], [len(t) for t in c['gts']]
    assert min(lens_p) == 1 and min(lens_g) == 1 and (~c['common']).sum() > 100 and c['common'].sum() > 1000
    best = c['oracle'].max(1)
    spread = best[:40]
    print(f'max IoU fixture: {int(c["common"].sum())} common-frame pairs of {P * G}; best oracle IoU of the jittered copies '
          f'{spread.min():.3f} ... {spread.max():.3f}; exact copy {best[40]:.6f}')
    assert spread.min() < 0.35 and spread.max() > 0.9 and best[40] > 0.9999 and best[41:56].max() == 0
    # first yardstick: the parent's kernel through Tracklet.intersection_ious, to the last bit
    assert np.array_equal(c['got'].view(np.uint32), c['parent'].view(np.uint32))
    assert (c['got'][~c['common']] == 0).all()
    # second: the C oracle, within twice what the parent's kernel itself deviates on this fixture
    dev_parent = float(np.abs(c['parent'] - c['oracle'])[c['common']].max())
    dev_new = float(np.abs(c['got'] - c['oracle'])[c['common']].max())
    print(f'largest deviation from the oracle: parent kernel {dev_parent:.3e}, ococc_tracklet_max_iou_f32 {dev_new:.3e}')
    assert dev_new <= 2 * dev_parent


def test_candidates_equal_parent_and_oracle(iou_case, dev):
    from objectcentricocccompletion_amd import ctrl_prep as cp
    c = iou_case
    got = cp.segment_candidates(c['pds'], c['gts'], 0.5, dev)
    names = lambda picked: [[c['gts'][j].id for j in row] for row in picked]
    assert names(got) == names([np.nonzero(row > 0.5)[0].tolist() for row in c['parent']])      # ids and order, no band
    band = float(np.abs(c['parent'] - c['oracle'])[c['common']].max())
    unsure = c['common'] & (np.abs(c['oracle'] - 0.5) <= band)
    print(f'candidates: {int(unsure.sum())} of {int(c["common"].sum())} common-frame pairs within {band:.3e} of 0.5; '
          f'{sum(len(r) for r in got)} candidates')
    assert unsure.sum() <= 0.01 * c['common'].sum()
    picked = np.zeros(c['oracle'].shape, bool)
    for i, row in enumerate(got):
        picked[i, row] = True
    assert np.array_equal(picked[~unsure], (c['oracle'] > 0.5)[~unsure])
    assert 20 <= sum(len(r) for r in got) <= 45


# ---------------------------------------------------------------------------------------------- end to end
def _run(cmd, timeout):
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def test_raw_to_training_end_to_end(tmp_path, dev):
    from objectcentricocccompletion_amd.dataset import WaymoTrackletDatasetWithOcc
    outs = {}
    for process in (1, 2):
        raw = str(tmp_path / f'raw{process}')
        _run([sys.executable, 'tools/make_synthetic_raw.py', raw], 300)
        cfg = os.path.join(raw, 'synthetic_vehicle.yaml')
        _run([sys.executable, 'tools/ctrl/generate_track_input.py', cfg, '--process', str(process)], 600)
        log = _run([sys.executable, 'tools/ctrl/generate_candidates.py', cfg, '--gt-bin-path',
                    os.path.join(raw, 'waymo_format', 'train_gt.bin'), '--process', str(process)], 600)
        assert 'Tracklet FP rate: 0.25' in log and 'Box FP rate:' in log and 'Average candidates per trk 0.75' in log
        outs[process] = raw
    stem = os.path.join('tracklet_data', 'synthetic_vehicle_training')
    for name in (stem + '.pkl', stem + '_gt_candidates.pkl'):
        one, two = (open(os.path.join(outs[p], name), 'rb').read() for p in (1, 2))
        assert one == two, f'{name} differs between --process 1 and --process 2'
    raw = outs[1]
    info, cand = os.path.join(raw, stem + '.pkl'), os.path.join(raw, stem + '_gt_candidates.pkl')
    infos, cands = pickle.load(open(info, 'rb')), pickle.load(open(cand, 'rb'))
    assert len(infos) == len(cands) == 8
    for e, c in zip(infos, cands):
        for r in outs.values():
            pts = np.load(os.path.join(r, stem + '_database', f'{e[0]}--{e[1]}.npy'), allow_pickle=True)
            assert [len(p) for p in pts] == e[7] and all(p.shape[1] == 6 and p.dtype == np.float32 for p in pts)
        assert [g[1] for g in c] == ([] if e[1].endswith('_fp') else [e[1].replace('trk', 'gt')])
    j = lambda p: os.path.join(raw, p)
    ds = WaymoTrackletDatasetWithOcc(raw, cand, info, j('occ_gt'), j('poses.pkl'), pipeline=None, classes=['Car'],
                                     min_tracklet_points=100, min_tracklet_length=32)
    assert len(ds) == 6
    log = _run([sys.executable, 'tools/train.py', CFG, '--data-root', raw, '--iters', '2', '--work-dir', str(tmp_path / 'work'),
                '--proposals', stem + '.pkl', '--candidates', stem + '_gt_candidates.pkl'], 900)
    lines = [l for l in log.splitlines() if l.startswith('iter ')]
    assert len(lines) == 2
    for l in lines:
        vals = [float(l.split(f' {k} ')[1].split()[0]) for k in ('loss', 'cls', 'bbox', 'occ')]
        assert np.isfinite(vals).all(), l
