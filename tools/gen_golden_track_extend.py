"""Generate tests/golden/track_extend.npz: the REFERENCE's own track extension on a seeded fixture --
LiDARTracklet.set_poses / frame_transform / set_velocity / extend / extend_all / shared2ego(inplace=True)
(mmdet3d/core/bbox/structures/lidar_tracklet.py:345-387, 452-498, 638-652, 669-791), driven as
tools/ctrl/extend_tracks.py:156-190 drives them, imported unchanged through oracle/ref_train_shim.py where the reference
tree exists.  Data only, no reference source.

Inputs: 2 segments of 60 frames, poses some kilometres from the origin, turning (with a little pitch and roll); 40
tracklets that cover every branch: shorter than the minimum length, a single box, a first gap of exactly 500 000 and of
500 001 microseconds, a start at frame 0 (nothing to add) and at frame 3 (length clipped), a gap inside the tracklet,
extend_all reaching and not reaching the segment's end, a velocity window larger than the tracklet, a length of exactly
min_length_to_extend_all.  Two cases over the same tracklets: plain `extend`, and `extend_all`.

Also measured here and stored as `margin`: the largest distance (metres for the centres, radians modulo 2 pi for the
yaw) between the reference's float32 chain and the float64 restatement of tests/test_gpu_track_extend.py on this
fixture.  The GPU test holds the kernel to twice that.  Above 5 cm something other than rounding is wrong: no file is
written.

usage: python tools/gen_golden_track_extend.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

T = 60
CONFIGS = {   # extend_length, min_length_to_extend, extend_all, min_length_to_extend_all, velo_window_size; multiplier
    'extend': ((10, 3, 0, 0, 10), 0.9),
    'extend_all': ((10, 3, 1, 6, 10), 0.8),
}


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    m = np.eye(3)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def make_inputs(seed=7):
    rng = np.random.default_rng(seed)
    poses, stamps = [], []
    for s in range(2):
        ts = [1_550_000_000_000_000 * (s + 1) + 100_000 * f for f in range(T)]
        if s == 1:
            ts = [v + int(rng.integers(-3000, 3000)) for v in ts]
            ts[20], ts[25] = ts[20] - ts[20] % 100_000, ts[20] - ts[20] % 100_000 + 500_001    # a gap of 500 001
            ts[30], ts[35] = ts[30] - ts[30] % 100_000, ts[30] - ts[30] % 100_000 + 500_000    # a gap of exactly 500 000
        assert ts == sorted(ts) and len(set(ts)) == T
        stamps.append(ts)
        origin = np.array([3000.0 + 1500 * s, -4500.0 + 800 * s, 40.0])
        seg = []
        for f in range(T):
            p = np.eye(4)
            p[:3, :3] = rot(2, 0.5 + 0.025 * f * (1 - 2 * s)) @ rot(1, 0.01 * np.sin(0.2 * f)) @ rot(0, 0.008 * np.cos(0.15 * f))
            p[:3, 3] = origin + [9.0 * f, 0.08 * f * f * (1 - 2 * s), 0.02 * f]
            seg.append(p.astype(np.float32))
        poses.append(np.stack(seg, 0))
    # the frames of every tracklet, per segment the same catalogue of branches
    catalogue = [
        [5, 6],                                   # shorter than min_length
        [17],                                     # one box
        list(range(0, 14)),                       # starts at frame 0: nothing to add in front
        list(range(3, 20)),                       # starts at frame 3: length clipped to 3
        list(range(12, 40)),                      # plain
        [15, 16, 17, 21, 22, 26, 27, 28, 29],     # gaps inside
        list(range(22, T)),                       # to the segment's end: extend_all adds nothing behind
        list(range(14, 50)),                      # extend_all adds frames on both sides
        [20, 25, 26, 27, 28, 29, 30, 31],         # first gap 5 frames (segment 1: 500 001 us, not extended)
        [30, 35, 36, 37, 38, 39, 40, 41, 42],     # first gap 5 frames (segment 1: exactly 500 000 us, extended)
        [40, 41, 42, 43],                         # window larger than the tracklet
        [11, 12, 13, 14, 15, 16],                 # exactly min_length_to_extend_all boxes: plain extend
        [11, 12, 13, 14, 15, 16, 17],             # one more: extend_all
        [2, 4, 6],                                # exactly min_length, uneven steps, clipped to 2
        [T - 3, T - 2, T - 1],                    # the last frames
        [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30],
    ]
    boxes, scores, offsets, frames, segments = [], [], [0], [], []
    for s in range(2):
        for k in range(20):
            fr = catalogue[k] if k < len(catalogue) else sorted(rng.choice(T, int(rng.integers(3, 45)), replace=False).tolist())
            # an object moving in the world at constant velocity (with noise), expressed in every frame's ego pose
            start = poses[s][fr[0]][:3, 3].astype(np.float64) + np.append(rng.uniform(-60, 60, 2), rng.uniform(-2, 1))
            velo = np.append(rng.uniform(-12, 12, 2), 0.0)
            yaw_w = rng.uniform(-np.pi, np.pi)
            size = [rng.uniform(1.7, 2.3), rng.uniform(4.0, 5.5), rng.uniform(1.4, 2.0)]
            for f in fr:
                p = poses[s][f].astype(np.float64)
                world = start + velo * ((stamps[s][f] - stamps[s][fr[0]]) / 1e6) + rng.normal(0, 0.05, 3)
                inv = np.linalg.inv(p)
                c = inv[:3, :3] @ world + inv[:3, 3]
                h = inv[:3, :3] @ np.array([np.sin(yaw_w), np.cos(yaw_w), 0.0])
                boxes.append([c[0], c[1], c[2], *size, np.arctan2(h[0], h[1]) + rng.normal(0, 0.01)])
                scores.append(float(np.float32(rng.uniform(0.2, 1.0))))
            frames += fr
            offsets.append(len(frames))
            segments.append(s)
    return dict(boxes=np.asarray(boxes, np.float32), scores=np.asarray(scores, np.float64), offsets=np.asarray(offsets, np.int64),
                frames=np.asarray(frames, np.int64), segments=np.asarray(segments, np.int64),
                poses=np.concatenate(poses, 0).reshape(-1, 16), timestamps=np.asarray(stamps[0] + stamps[1], np.int64),
                seg_offsets=np.asarray([0, T, 2 * T], np.int64))


def run_reference(fx, config, multiplier):
    from oracle import ref_train_shim as S
    Trk = S.load_train_classes()['Tracklet']
    extend_length, min_length, extend_all, min_all, window = config
    ts2pose = {int(ts): torch.from_numpy(p.reshape(4, 4).copy()).float() for ts, p in zip(fx['timestamps'], fx['poses'])}
    out_boxes, out_scores, out_ts, out_offsets = [], [], [], [0]
    for t in range(len(fx['segments'])):
        lo, hi = fx['offsets'][t], fx['offsets'][t + 1]
        s0, s1 = fx['seg_offsets'][fx['segments'][t]], fx['seg_offsets'][fx['segments'][t] + 1]
        full_ts = [int(v) for v in fx['timestamps'][s0:s1]]
        trk = Trk(f'segment-{fx["segments"][t]}', f'trk{t}', 1, False, box_list=[fx['boxes'][i:i + 1].copy() for i in range(lo, hi)],
                  ts_list=[full_ts[f] for f in fx['frames'][lo:hi]], score_list=[float(v) for v in fx['scores'][lo:hi]])
        trk.freeze()
        trk.set_poses(ts2pose)
        trk.frame_transform(trk.pose_list[0])
        trk.set_velocity()
        if extend_all and len(trk) > min_all:
            trk.extend_all(full_ts, min_all, ts2pose, multiplier, window)
        else:
            trk.extend(extend_length, 'backward', full_ts, min_length, ts2pose, multiplier, window)
        trk.shared2ego(inplace=True)
        out_boxes.append(torch.stack([b.tensor.reshape(-1) for b in trk.box_list], 0).numpy())
        out_scores += [float(v) for v in trk.score_list]
        out_ts += list(trk.ts_list)
        out_offsets.append(len(out_ts))
    return dict(out_boxes=np.concatenate(out_boxes, 0).astype(np.float32), out_scores=np.asarray(out_scores, np.float64),
                out_timestamps=np.asarray(out_ts, np.int64), out_offsets=np.asarray(out_offsets, np.int32))


def main():
    from test_gpu_track_extend import extend_f64, wrapped
    fx = make_inputs()
    out = dict(fx)
    margin = 0.0
    for case, (config, multiplier) in CONFIGS.items():
        ref = run_reference(fx, config, multiplier)
        cfg = dict(extend_length=config[0], min_length=config[1], extend_all=bool(config[2]), min_length_all=config[3],
                   velo_window_size=config[4], score_multiplier=multiplier)
        exp = extend_f64(fx, cfg)
        assert [len(e[0]) for e in exp] == np.diff(ref['out_offsets']).tolist(), 'the restatement plans differently'
        d = np.abs(wrapped(np.concatenate([e[0] for e in exp], 0) - ref['out_boxes'].astype(np.float64)))
        print(f'{case}: {len(d)} boxes from {len(fx["boxes"])}; reference float32 chain vs float64 restatement: '
              f'centres {d[:, :3].max():.3e} m, yaw {d[:, 6].max():.3e} rad')
        margin = max(margin, float(d[:, [0, 1, 2, 6]].max()))
        out[f'{case}_config'] = np.asarray(config, np.int64)
        out[f'{case}_score_multiplier'] = np.float64(multiplier)
        out.update({f'{case}_{k}': v for k, v in ref.items()})
    assert margin <= 0.05, f'{margin} m between the reference and the restatement is not rounding: find the cause'
    out['margin'] = np.float64(margin)
    path = os.path.join(ROOT, 'tests', 'golden', 'track_extend.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path)} bytes), margin {margin:.3e}')


if __name__ == '__main__':
    main()
