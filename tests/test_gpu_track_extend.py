"""Track extension on the MI355X (csrc/track_extend.hip, ctrl_prep.extend_tracks_packed) against

  * a float64 restatement of the rules written in this file (extend_f64: numpy, poses promoted from float32), and
  * tests/golden/track_extend.npz, captured from the reference's own LiDARTracklet by tools/gen_golden_track_extend.py.

Bounds.  Boxes against the restatement: 1 ulp of float32 at max(|value|, 1) -- the kernel computes in float64 and rounds
once on store (half an ulp); the other half covers atan2 / product-order differences between device and numpy doubles.
Yaw is compared modulo 2 pi.  Scores: 1e-12 relative (two pow implementations that are each good to an ulp of float64).
Boxes against the golden: twice the largest distance between the golden (the reference's float32 chain) and the
restatement on this fixture, measured on the CPU when the golden was generated and stored in the file (`margin`;
DESIGN.md quotes it); frame indices, lengths and branch decisions exact."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'track_extend.npz')
CASES = ('extend', 'extend_all')


# ---------------------------------------------------------------------------------------------- float64 restatement
def affine_inverse(p):
    """inverse of [R t; 0 0 0 1] in float64, R inverted as a general 3x3"""
    out = np.eye(4)
    out[:3, :3] = np.linalg.inv(p[:3, :3])
    out[:3, 3] = -out[:3, :3] @ p[:3, 3]
    return out


def move(mm, box):
    """(x, y, z, yaw) through the 4x4 mm: the centre as a point, the yaw from the heading vector (sin, cos, 0)"""
    c = mm[:3, :3] @ box[:3] + mm[:3, 3]
    h = mm[:3, :3] @ np.array([np.sin(box[3]), np.cos(box[3]), 0.0])
    return np.array([c[0], c[1], c[2], np.arctan2(h[0], h[1])])


def plan_f64(length, first, last, stamps, ts, cfg):
    """(frames added in front, behind) of one tracklet, straight from the rules"""
    use_all = cfg['extend_all'] and length > cfg['min_length_all']
    if length < (cfg['min_length_all'] if use_all else cfg['min_length']) or length < 2:
        return 0, 0
    if ts[1] - ts[0] > 500_000:
        return 0, 0
    if use_all:
        return first, len(stamps) - 1 - last
    return min(cfg['extend_length'], first), 0


def extend_f64(fx, cfg):
    """fx: the fixture's inputs (arrays of the .npz) -> per tracklet (boxes [L', 7] float64, scores [L'], frames [L'])"""
    out = []
    for t in range(len(fx['segments'])):
        lo, hi = fx['offsets'][t], fx['offsets'][t + 1]
        s0, s1 = fx['seg_offsets'][fx['segments'][t]], fx['seg_offsets'][fx['segments'][t] + 1]
        poses = fx['poses'][s0:s1].astype(np.float64).reshape(-1, 4, 4)
        stamps = [int(v) for v in fx['timestamps'][s0:s1]]
        fr = [int(v) for v in fx['frames'][lo:hi]]
        ego = fx['boxes'][lo:hi].astype(np.float64)
        sc = fx['scores'][lo:hi].astype(np.float64)
        ts = [stamps[f] for f in fr]
        length = hi - lo
        to_shared = affine_inverse(poses[fr[0]])
        shared = np.stack([move(to_shared @ poses[f], ego[i, [0, 1, 2, 6]]) for i, f in enumerate(fr)], 0)
        back, fwd = plan_f64(length, fr[0], fr[-1], stamps, ts, cfg)
        rows = [(shared[i], ego[i, 3:6], f, sc[i]) for i, f in enumerate(fr)]
        if back or fwd:
            velo = np.diff(shared[:, :2], axis=0) / (np.diff(np.asarray(ts, np.float64)) / 1e6)[:, None]
            velo = np.concatenate([velo[:1], velo], 0)                    # row 0 duplicates row 1
            window = min(cfg['velo_window_size'], length)
            head = []
            v = velo[:window].mean(0)
            for i in range(back):
                f = fr[0] - back + i
                b = shared[0].copy()
                b[:2] += v * ((stamps[f] - ts[0]) / 1e6)
                head.append((b, ego[0, 3:6], f, sc[0] * cfg['score_multiplier'] ** (i + 1)))
            tail = []
            v = velo[-window:].mean(0)
            for i in range(fwd):
                f = fr[-1] + 1 + i
                b = shared[-1].copy()
                b[:2] += v * ((stamps[f] - stamps[fr[-1] + 1]) / 1e6)   # from the first extended frame
                tail.append((b, ego[-1, 3:6], f, sc[-1] * cfg['score_multiplier'] ** (i + 1)))
            rows = head + rows + tail
        boxes = np.zeros((len(rows), 7))
        for k, (b, size, f, _) in enumerate(rows):
            e = move(affine_inverse(poses[f]) @ poses[fr[0]], b)
            boxes[k] = [e[0], e[1], e[2], size[0], size[1], size[2], e[3]]
        out.append((boxes, np.array([r[3] for r in rows]), np.array([r[2] for r in rows], np.int64)))
    return out


def wrapped(d):
    """differences with column 6 (yaw) taken modulo 2 pi"""
    d = np.array(d, np.float64)
    d[..., 6] = (d[..., 6] + np.pi) % (2 * np.pi) - np.pi
    return d


def load_fixture():
    z = np.load(GOLDEN)
    fx = {k: z[k] for k in z.files}
    cfgs = {}
    for case in CASES:
        c = fx[f'{case}_config']
        cfgs[case] = dict(extend_length=int(c[0]), min_length=int(c[1]), extend_all=bool(c[2]), min_length_all=int(c[3]),
                          velo_window_size=int(c[4]), score_multiplier=float(fx[f'{case}_score_multiplier']))
    return fx, cfgs


# ---------------------------------------------------------------------------------------------- the device side
def run_kernel(fx, cfg, dev, tracklets=None):
    """the kernel on the fixture (or on the tracklets listed) -> (boxes, scores, frames, out_offsets) as numpy"""
    from objectcentricocccompletion_amd import ctrl_prep as cp
    pick = list(range(len(fx['segments']))) if tracklets is None else list(tracklets)
    lens = [int(fx['offsets'][t + 1] - fx['offsets'][t]) for t in pick]
    rows = np.concatenate([np.arange(fx['offsets'][t], fx['offsets'][t + 1]) for t in pick])
    offsets = np.concatenate([[0], np.cumsum(lens)])
    seg_ts = [[int(v) for v in fx['timestamps'][a:b]] for a, b in zip(fx['seg_offsets'], fx['seg_offsets'][1:])]
    back, fwd, out_offsets = cp.plan_extension(offsets, fx['frames'][rows], fx['segments'][pick], seg_ts, cfg['extend_length'],
                                               cfg['min_length'], cfg['extend_all'], cfg['min_length_all'])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    boxes, scores, frames = cp.extend_tracks_packed(up(fx['boxes'][rows]), offsets, fx['frames'][rows], fx['segments'][pick],
                                                    up(fx['scores'][rows]), up(fx['poses']), up(fx['timestamps']),
                                                    fx['seg_offsets'], back, fwd, out_offsets, cfg['score_multiplier'],
                                                    cfg['velo_window_size'])
    torch.cuda.synchronize()
    return boxes.cpu().numpy(), scores.cpu().numpy(), frames.cpu().numpy(), out_offsets


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_kernel_equals_f64_restatement(dev, case):
    fx, cfgs = load_fixture()
    boxes, scores, frames, oo = run_kernel(fx, cfgs[case], dev)
    assert boxes.dtype == np.float32 and scores.dtype == np.float64 and frames.dtype == np.int32
    exp = extend_f64(fx, cfgs[case])
    assert oo[-1] == sum(len(e[0]) for e in exp) == len(boxes)
    worst_ulp, worst_score = 0.0, 0.0
    for t, (eb, es, ef) in enumerate(exp):
        got = slice(oo[t], oo[t + 1])
        assert np.array_equal(frames[got], ef), f'tracklet {t}: frame indices'
        ulp = np.spacing(np.maximum(np.abs(eb), 1.0).astype(np.float32)).astype(np.float64)
        d = np.abs(wrapped(boxes[got].astype(np.float64) - eb))
        worst_ulp = max(worst_ulp, float((d / ulp).max()))
        worst_score = max(worst_score, float((np.abs(scores[got] - es) / np.abs(es)).max()))
    print(f'{case}: {len(boxes)} boxes; farthest box coordinate {worst_ulp:.3f} ulp of float32 from the float64 restatement; '
          f'scores within {worst_score:.2e} relative')
    assert worst_ulp <= 1.0
    assert worst_score <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_kernel_against_reference_golden(dev, case):
    fx, cfgs = load_fixture()
    boxes, scores, frames, oo = run_kernel(fx, cfgs[case], dev)
    margin = 2 * float(fx['margin'])
    assert 0 < margin < 0.10            # (the generator refuses a measured distance above 5 cm)
    g_off = fx[f'{case}_out_offsets']
    assert np.array_equal(oo, g_off), 'output lengths / branch decisions'
    seg_of_box = np.repeat(fx['segments'], np.diff(oo))
    stamps = fx['timestamps'][fx['seg_offsets'][seg_of_box] + frames]
    assert np.array_equal(stamps, fx[f'{case}_out_timestamps'])
    d = np.abs(wrapped(boxes.astype(np.float64) - fx[f'{case}_out_boxes'].astype(np.float64)))
    print(f'{case}: largest distance to the reference golden {d.max():.3e} (margin {margin:.3e} = 2 x {float(fx["margin"]):.3e})')
    assert d.max() <= margin
    assert np.array_equal(boxes[:, 3:6], fx[f'{case}_out_boxes'][:, 3:6])          # sizes are copied
    # the reference's scores are Python floats: s * m ** (i + 1)
    assert np.allclose(scores, fx[f'{case}_out_scores'], rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_same_bytes_twice_and_per_segment(dev):
    fx, cfgs = load_fixture()
    for case in CASES:
        one = run_kernel(fx, cfgs[case], dev)
        two = run_kernel(fx, cfgs[case], dev)
        for a, b in zip(one, two):
            assert a.tobytes() == b.tobytes()
        parts = []
        for s in range(len(fx['seg_offsets']) - 1):
            pick = np.nonzero(fx['segments'] == s)[0]
            assert len(pick) > 5
            parts.append((pick, run_kernel(fx, cfgs[case], dev, pick)))
        for pick, (pb, ps, pf, po) in parts:
            for k, t in enumerate(pick):
                whole, part = slice(one[3][t], one[3][t + 1]), slice(po[k], po[k + 1])
                assert one[0][whole].tobytes() == pb[part].tobytes() and one[1][whole].tobytes() == ps[part].tobytes()
                assert np.array_equal(one[2][whole], pf[part])
