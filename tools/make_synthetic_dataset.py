"""Write a small synthetic tracklet dataset in the reference's on-disk formats (what WaymoTrackletDatasetWithOcc
reads, mmdet3d/datasets/waymo_tracklet_dataset.py:491-584): <root>/tracklet_data/synth_training.pkl (proposals),
synth_training_gt_candidates.pkl, synth_training_database/<segment>--<id>.npy (per-frame [n,6] points),
<root>/poses.pkl, <root>/occ_gt/<segment>/<id>.npz (key 'occ', X x Y x Z in {0,1,2}), and the detection ground truth
<root>/waymo_format/gt.bin (metrics.Objects with lidar point counts and difficulty levels, so that LEVEL_1, LEVEL_2 and
ignored objects all occur: what dataset.evaluate(metric='waymo_native') scores against).

usage: python tools/make_synthetic_dataset.py <root> [--tracklets 6] [--frames 40]"""
import argparse
import os
import pickle
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def write_gt_bin(waymo_dir, gt_tracklets):
    """<waymo_dir>/gt.bin from (segment, id, boxes [n, 7] LiDAR convention, timestamps, points per box).  No random draw:
    every tenth frame of an object is made LEVEL_2 by its difficulty level (frame 5, 15, ...), LEVEL_2 by a count of 3
    points (7, 17, ...) or ignored by a count of 0 (9, 19, ...); the other frames keep their point count (LEVEL_1)."""
    import torch
    from objectcentricocccompletion_amd import waymo_io
    from objectcentricocccompletion_amd.tracklet import Tracklet
    os.makedirs(waymo_dir, exist_ok=True)
    trks, points, levels = [], [], []
    for seg, tid, boxes, ts, num_pts in gt_tracklets:
        trks.append(Tracklet(torch.from_numpy(np.asarray(boxes, np.float32)), list(ts), torch.ones(len(ts)), 0, seg, tid))
        points.append([3 if f % 10 == 7 else 0 if f % 10 == 9 else int(n) for f, n in enumerate(num_pts)])
        levels.append([2 if f % 10 == 5 else 1 for f in range(len(ts))])
    return waymo_io.convert_tracklet_to_waymo(trks, os.path.join(waymo_dir, 'gt.bin'), ('Car', 'Pedestrian', 'Cyclist'),
                                              None, levels, points)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('root')
    ap.add_argument('--tracklets', type=int, default=6)
    ap.add_argument('--frames', type=int, default=40)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args(argv)
    rng = np.random.default_rng(a.seed)
    tdir = os.path.join(a.root, 'tracklet_data')
    db = os.path.join(tdir, 'synth_training_database')
    os.makedirs(db, exist_ok=True)
    proposals, candidates, poses, gt_tracklets = [], [], {}, []
    for t in range(a.tracklets):
        seg, tid = f'segment-{t // 3:03d}', f'obj{t:03d}'
        ts = [1_000_000 * (t + 1) + 100_000 * f for f in range(a.frames)]
        size = np.array([rng.uniform(1.7, 2.2), rng.uniform(4.0, 5.2), rng.uniform(1.4, 1.9)])
        boxes, pts = [], []
        for f, stamp in enumerate(ts):
            yaw = 0.02 * f + rng.normal(0, 0.01)
            pose = np.eye(4)
            pose[:3, :3] = rot_z(0.01 * f)
            pose[:3, 3] = [1.5 * f, 0.05 * f * f, 0]
            poses[stamp] = pose.astype(np.float32)
            ctr = np.array([12 + 0.3 * f, -4 + 0.1 * f, 0.1])           # in that frame's ego coordinates
            box = np.concatenate([ctr, size, [yaw]]).astype(np.float32)
            boxes.append(box)
            n = int(rng.integers(150, 400))
            local = (rng.random((n, 3)) - 0.5) * size * [1, 1, 1]         # points inside the box, box frame
            world = local @ rot_z(yaw).T + ctr + [0, 0, size[2] / 2]
            attr = rng.random((n, 3)).astype(np.float32)                  # intensity, elongation, (wrong) timestamp
            pts.append(np.concatenate([world, attr], 1).astype(np.float32))
        gt = [b + rng.normal(0, [0.05, 0.05, 0.02, 0.02, 0.02, 0.02, 0.01]).astype(np.float32) for b in boxes]
        far = [b + np.array([25, 25, 0, 0, 0, 0, 0], np.float32) for b in boxes]
        num_pts = [len(p) for p in pts]
        proposals.append((seg, tid, 1, False, [b[None] for b in boxes], ts, rng.uniform(0.3, 1.0, a.frames).tolist(), num_pts))
        candidates.append([(seg, tid + '_far', 1, False, [b[None] for b in far], ts, [1.0] * a.frames, num_pts),
                           (seg, tid + '_gt', 1, False, [b[None] for b in gt], ts, [1.0] * a.frames, num_pts)])
        gt_tracklets.append((seg, tid + '_gt', np.stack(gt), ts, num_pts))
        arr = np.empty(len(pts), dtype=object)
        for i, p in enumerate(pts):
            arr[i] = p
        np.save(os.path.join(db, f'{seg}--{tid}.npy'), arr, allow_pickle=True)
        for name in (tid + '_gt', tid + '_far'):
            dims = np.ceil(size / 0.2).astype(int)
            occ = rng.integers(0, 3, dims).astype(np.int64)
            os.makedirs(os.path.join(a.root, 'occ_gt', seg), exist_ok=True)
            np.savez_compressed(os.path.join(a.root, 'occ_gt', seg, f'{name}.npz'), occ=occ)
    with open(os.path.join(tdir, 'synth_training.pkl'), 'wb') as f:
        pickle.dump(proposals, f)
    with open(os.path.join(tdir, 'synth_training_gt_candidates.pkl'), 'wb') as f:
        pickle.dump(candidates, f)
    with open(os.path.join(a.root, 'poses.pkl'), 'wb') as f:
        pickle.dump(poses, f)
    write_gt_bin(os.path.join(a.root, 'waymo_format'), gt_tracklets)
    print('wrote', a.tracklets, 'tracklets x', a.frames, 'frames under', a.root)


if __name__ == '__main__':
    main()
