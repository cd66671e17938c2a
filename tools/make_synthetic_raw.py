"""Write a small synthetic RAW tree, the input of the tracklet data preparation (tools/ctrl/generate_track_input.py,
tools/ctrl/generate_candidates.py), so that the chain raw -> track input -> candidates -> tools/train.py --data-root
runs without Waymo data:

    <out>/waymo_format/pred.bin, train_gt.bin      tracking result and ground truth (waymo_io's own writer)
    <out>/waymo_format/gt.bin                      the same ground truth with lidar point counts and difficulty levels
                                                   (LEVEL_1, LEVEL_2 and ignored objects: tools/waymo_detection_metrics.py)
    <out>/kitti_format/idx2timestamp.pkl, idx2contextname.pkl, training/velodyne/<idx>.bin   ([n, 6] float32 clouds)
    <out>/synthetic_vehicle.yaml                   tools/ctrl/data_configs/synthetic_vehicle.yaml with this tree's paths
    <out>/synthetic_extend.yaml                    tools/ctrl/data_configs/synthetic_extend.yaml with this tree's paths
    <out>/poses.pkl, <out>/occ_gt/<segment>/<gt id>.npz    what the dataset class needs besides (as make_synthetic_dataset.py)

usage: python tools/make_synthetic_raw.py <out> [--segments 2] [--tracklets 3] [--frames 40]
then:  python tools/ctrl/generate_track_input.py <out>/synthetic_vehicle.yaml
       python tools/ctrl/generate_candidates.py <out>/synthetic_vehicle.yaml --gt-bin-path <out>/waymo_format/train_gt.bin
       python tools/train.py configs/ococcnet_mi355x.py --data-root <out> \\
           --proposals tracklet_data/synthetic_vehicle_training.pkl \\
           --candidates tracklet_data/synthetic_vehicle_training_gt_candidates.pkl"""
import argparse
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from make_synthetic_dataset import rot_z  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('--segments', type=int, default=2)
    ap.add_argument('--tracklets', type=int, default=3, help='objects per segment')
    ap.add_argument('--frames', type=int, default=40)
    ap.add_argument('--background', type=int, default=3000, help='points per frame outside the objects')
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args(argv)
    import torch
    import yaml
    from objectcentricocccompletion_amd import waymo_io
    from objectcentricocccompletion_amd.tracklet import Tracklet
    rng = np.random.default_rng(a.seed)
    out = os.path.abspath(a.out)
    velo = os.path.join(out, 'kitti_format', 'training', 'velodyne')
    for d in (velo, os.path.join(out, 'waymo_format'), os.path.join(out, 'tracklet_data')):
        os.makedirs(d, exist_ok=True)
    idx2ts, idx2seg, poses, preds, gts, gt_points, gt_levels = {}, {}, {}, [], [], [], []
    for s in range(a.segments):
        seg = f'segment-{s:03d}'
        ts = [10_000_000 * (s + 1) + 100_000 * f for f in range(a.frames)]
        clouds = [[(rng.uniform([-60, -60, -1], [60, 60, 4], (a.background, 3)))] for _ in ts]
        attrs = lambda n: rng.random((n, 3))          # intensity, elongation, (wrong) timestamp
        for f, stamp in enumerate(ts):
            pose = np.eye(4)
            pose[:3, :3] = rot_z(0.01 * f)
            pose[:3, 3] = [1.5 * f, 0.05 * f * f, 0]
            poses[stamp] = pose.astype(np.float32)
        for t in range(a.tracklets):
            size = np.array([rng.uniform(1.7, 2.2), rng.uniform(4.0, 5.2), rng.uniform(1.4, 1.9)])
            first = int(rng.integers(0, 4)) if t else 0       # objects appear at different frames
            boxes, counts = [], []
            for f in range(first, a.frames):
                yaw = 0.02 * f + rng.normal(0, 0.01) + 0.7 * t
                ctr = np.array([12 + 0.3 * f, -14 + 12 * t + 0.1 * f, 0.1])    # in that frame's ego coordinates
                boxes.append(np.concatenate([ctr, size, [yaw]]))
                n = int(rng.integers(150, 400))
                counts.append(n)
                local = (rng.random((n, 3)) - 0.5) * size
                # (box convention of the kernels: w along x at yaw 0, turned CLOCKWISE by yaw, as make_synthetic_dataset.py)
                clouds[f].append(local @ rot_z(yaw).T + ctr + [0, 0, size[2] / 2])
            gt = np.stack(boxes).astype(np.float32)
            pd = (gt + rng.normal(0, [0.05, 0.05, 0.02, 0.02, 0.02, 0.02, 0.01], gt.shape)).astype(np.float32)
            stamps = ts[first:]
            gts.append(Tracklet(torch.from_numpy(gt), stamps, None, 0, seg, f'gt{s}_{t:02d}'))
            # gt.bin only: every tenth frame LEVEL_2 by difficulty, LEVEL_2 by 3 points, ignored by 0 points
            gt_points.append([3 if f % 10 == 7 else 0 if f % 10 == 9 else c for f, c in enumerate(counts)])
            gt_levels.append([2 if f % 10 == 5 else 1 for f in range(len(counts))])
            preds.append(Tracklet(torch.from_numpy(pd), stamps, torch.from_numpy(rng.uniform(0.3, 1.0, len(pd)).astype(np.float32)),
                                  0, seg, f'trk{s}_{t:02d}'))
            dims = np.ceil(size / 0.2).astype(int)
            os.makedirs(os.path.join(out, 'occ_gt', seg), exist_ok=True)
            np.savez_compressed(os.path.join(out, 'occ_gt', seg, f'gt{s}_{t:02d}.npz'), occ=rng.integers(0, 3, dims).astype(np.int64))
        # one false positive without any ground truth nearby and above every point: no candidates, no points
        fp = np.tile(np.array([[-30, 30, 20, 2, 4.5, 1.6, 0.3]], np.float32), (a.frames, 1))
        preds.append(Tracklet(torch.from_numpy(fp), ts, torch.full((a.frames,), 0.2), 0, seg, f'trk{s}_fp'))
        for f, stamp in enumerate(ts):
            idx = f'{s:01d}{f:06d}'
            idx2ts[idx], idx2seg[idx] = stamp, seg
            xyz = np.concatenate(clouds[f], 0)
            np.concatenate([xyz, attrs(len(xyz))], 1).astype(np.float32).tofile(os.path.join(velo, idx + '.bin'))
    waymo_io.convert_tracklet_to_waymo(preds, os.path.join(out, 'waymo_format', 'pred.bin'))
    waymo_io.convert_tracklet_to_waymo(gts, os.path.join(out, 'waymo_format', 'train_gt.bin'))
    waymo_io.convert_tracklet_to_waymo(gts, os.path.join(out, 'waymo_format', 'gt.bin'), detection_difficulty_level=gt_levels,
                                       num_lidar_points_in_box=gt_points)
    for name, obj in (('idx2timestamp.pkl', idx2ts), ('idx2contextname.pkl', idx2seg)):
        with open(os.path.join(out, 'kitti_format', name), 'wb') as f:
            pickle.dump(obj, f)
    with open(os.path.join(out, 'poses.pkl'), 'wb') as f:
        pickle.dump(poses, f)
    with open(os.path.join(ROOT, 'tools', 'ctrl', 'data_configs', 'synthetic_vehicle.yaml')) as f:
        cfg = yaml.safe_load(f)
    cfg.update(bin_path=os.path.join(out, 'waymo_format', 'pred.bin'), val_bin_path=os.path.join(out, 'waymo_format', 'pred_val.bin'),
               data_root=os.path.join(out, 'tracklet_data'), mm_data_root=os.path.join(out, 'kitti_format'))
    with open(os.path.join(out, 'synthetic_vehicle.yaml'), 'w') as f:
        yaml.safe_dump(cfg, f, sort_keys=False)
    with open(os.path.join(ROOT, 'tools', 'ctrl', 'data_configs', 'synthetic_extend.yaml')) as f:
        ext = yaml.safe_load(f)
    ext.update(bin_path=os.path.join(out, 'waymo_format', 'pred.bin'), mm_data_root=os.path.join(out, 'kitti_format'),
               poses_path=os.path.join(out, 'poses.pkl'))
    with open(os.path.join(out, 'synthetic_extend.yaml'), 'w') as f:
        yaml.safe_dump(ext, f, sort_keys=False)
    print('wrote', a.segments, 'segments x', a.frames, 'frames,', len(preds), 'predicted /', len(gts), 'GT tracklets under', out)


if __name__ == '__main__':
    main()
