#!/usr/bin/env python3
"""One sensor frame into step rows, timed on the MI355X: scene_rows.scene_step_rows (csrc/scene_rows.hip: one count
launch, one read-back, one fill launch) against the composition of existing operators it replaces, on the same inputs --
ctrl_prep.crop_frames_packed (count launch, read-back, fill launch of indices), the ATen gathers of the points and of the
rows' decoration with repeat_interleave and cat, the ATen transform (three addcmul per coordinate), the range mask and
the even-pick cap as index arithmetic and a boolean-mask compaction.
    python tools/time_scene_rows.py [--points 150000] [--boxes 8 64 256] [--inside 500] [--reps 15] [--out FILE.md]
A synthetic frame: --points points, of which --inside per box lie in the box (so the cap of 1024 bites for none by
default; --inside 2000 makes it bite), the rest background; a rigid transform per box; the ococcnet range.  Both paths are
checked to give the same rows, warmed up, then timed alternately; a call is timed with device events around it and with
the host clock up to a device synchronise; median (min - max) of the repetitions.  A report, not a gate."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_occ_export import fmt, timed   # noqa: E402 (the same measuring functions)

RANGE = (-204.7, -204.7, -3.99, 204.7, 204.7, 7.99)


def frame(num_points, num_boxes, inside, dev, seed=0):
    import numpy as np
    import torch
    g = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(num_boxes)))
    boxes = np.array([[-70 + 140 * (b % side + 0.5) / side, -70 + 140 * (b // side + 0.5) / side, 0.1, 2.0, 4.6, 1.6,
                       g.uniform(-np.pi, np.pi)] for b in range(num_boxes)], np.float32)
    parts = []
    for b in boxes:
        rot = float(b[6]) + np.pi / 2
        lx, ly = (g.random(inside) - 0.5) * b[4], (g.random(inside) - 0.5) * b[3]
        parts.append(np.stack([b[0] + lx * np.cos(rot) + ly * np.sin(rot), b[1] - lx * np.sin(rot) + ly * np.cos(rot),
                               b[2] + g.random(inside) * b[5]], 1))
    rest = num_points - inside * num_boxes
    assert rest >= 0, 'more points inside the boxes than --points'
    parts.append(np.concatenate([g.uniform(-75, 75, (rest, 2)), g.uniform(-1, 4, (rest, 1))], 1))
    xyz = np.concatenate(parts)
    cloud = np.concatenate([xyz, g.random((len(xyz), 3))], 1)[g.permutation(len(xyz))].astype(np.float32)
    mats = np.zeros((num_boxes, 3, 4))
    for k in range(num_boxes):
        a = g.uniform(-0.3, 0.3)
        mats[k, :, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        mats[k, :, 3] = g.uniform(-20, 20, 3) * [1, 1, 0.01]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return T(cloud), T(boxes), T(g.uniform(0.3, 1.0, num_boxes).astype(np.float32)), T(mats.reshape(-1, 12).astype(np.float32))


def composition(points, boxes, scores, mats, extra_width, cap, rng_dev):
    """the same rows from the operators the package had before scene_rows.hip"""
    import torch
    from objectcentricocccompletion_amd import ctrl_prep
    from objectcentricocccompletion_amd.scene_rows import decoration
    n, dev = boxes.size(0), points.device
    counts, idx = ctrl_prep.crop_frames_packed(points, [0, points.size(0)], ctrl_prep.enlarged_boxes(boxes, extra_width), [0, n])
    row = torch.repeat_interleave(torch.arange(n, device=dev), counts.to(dev))
    src, m = points[idx], mats[row]
    xyz = torch.stack([torch.addcmul(torch.addcmul(torch.addcmul(m[:, 4 * c + 3], src[:, 0], m[:, 4 * c]), src[:, 1],
                                                   m[:, 4 * c + 1]), src[:, 2], m[:, 4 * c + 2]) for c in range(3)], 1)
    keep = ((xyz > rng_dev[:3]) & (xyz < rng_dev[3:])).all(1)
    xyz, row = xyz[keep], row[keep]
    feats = torch.cat([src[keep, 3:5], decoration(boxes, scores)[row]], 1)
    if cap > 0:
        per = torch.bincount(row, minlength=n)
        first = torch.cumsum(per, 0) - per
        j, mm = torch.arange(row.numel(), device=dev) - first[row], per[row]
        pick = (mm <= cap) | ((j + 1) * cap // mm > j * cap // mm)
        xyz, feats, row = xyz[pick], feats[pick], row[pick]
    return xyz, feats, row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--points', type=int, default=150000)
    ap.add_argument('--boxes', type=int, nargs='+', default=[8, 64, 256])
    ap.add_argument('--inside', type=int, default=500, help='points inside every box')
    ap.add_argument('--max-points', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the table to this markdown file')
    args = ap.parse_args()
    import torch
    from objectcentricocccompletion_amd.scene_rows import scene_step_rows
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is nothing to time without one'
    dev = torch.device('cuda:0')
    rng_dev = torch.tensor(RANGE, dtype=torch.float32, device=dev)
    lines = ['| points | boxes | rows | path | device events, ms: median (min - max) | host clock, ms |', '|---|---|---|---|---|---|']
    for n in args.boxes:
        points, boxes, scores, mats = frame(args.points, n, args.inside, dev)
        fused = lambda: scene_step_rows(points, boxes, scores, transforms=mats, extra_width=1.0, attr_dims=2,
                                        point_cloud_range=RANGE, max_points=args.max_points)[:3]
        parts = lambda: composition(points, boxes, scores, mats, 1.0, args.max_points, rng_dev)
        a, b = fused(), parts()
        same = all(torch.equal(x, y) for x, y in zip(a, b))
        close = a[0].shape == b[0].shape and torch.equal(a[2], b[2]) and bool(torch.allclose(a[0], b[0], rtol=0, atol=1e-4))
        assert close, 'the two paths disagree on the rows'
        print(f'{n} boxes: {a[0].size(0)} rows, bit-equal to the composition: {same}', flush=True)
        for _ in range(args.warmup):
            fused()
            parts()
        times = {'fused': ([], []), 'parts': ([], [])}
        for _ in range(args.reps):            # alternating: drift of the shared host hits both alike
            for name, fn in (('fused', fused), ('parts', parts)):
                e, h = timed(fn, 1)
                times[name][0].extend(e)
                times[name][1].extend(h)
        for name, what in (('fused', '`scene_step_rows`'), ('parts', 'crop + ATen gathers, transform, range, cap')):
            lines.append(f'| {args.points} | {n} | {a[0].size(0)} | {what} | {fmt(times[name][0])} | {fmt(times[name][1])} |')
            print(lines[-1], flush=True)
    text = '\n'.join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
