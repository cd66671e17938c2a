"""Timing of the tracklet data preparation kernels against the per-box / per-pair loops they replace
(profiles/ctrl_prep.md).  Needs the MI355X; no fallback.

  python tools/bench_ctrl_prep.py [--what crop|iou|all] [--repeat 5] [--loops 1]

crop: 200 frames x 150 000 points x 40 enlarged boxes, ctrl_prep.crop_frames_packed against, per box, a torch mask and
      nonzero on the device (the reference's loop, generate_track_input.py:84-99, minus its per-box copies).
iou:  P = 256 predicted, G = 128 GT tracklets over 200 frames, ctrl_prep.segment_candidates against a Python loop of
      Tracklet.intersection_ious(...).max().item() per pair (generate_candidates.py:61-65).
--loops 0 skips the loops (for a kernel trace of the new path alone).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def crop_case(frames, pts, nb, seed=0):
    rng = np.random.default_rng(seed)
    r, a = rng.uniform(5, 75, (frames, nb)), rng.uniform(-np.pi, np.pi, (frames, nb))
    boxes = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-1.5, 0.5, (frames, nb)), rng.uniform(3.6, 4.4, (frames, nb)),
                      rng.uniform(5.8, 7.5, (frames, nb)), rng.uniform(3.4, 4.0, (frames, nb)),
                      rng.uniform(-np.pi, np.pi, (frames, nb))], -1).astype(np.float32)
    half = pts // 2
    own = rng.integers(0, nb, (frames, half))
    near = np.take_along_axis(boxes[:, :, :3], own[:, :, None], 1) + [0, 0, 1.5] + rng.normal(0, [3, 3, 1.5], (frames, half, 3))
    far = rng.uniform([-80, -80, -3], [80, 80, 5], (frames, pts - half, 3))
    xyz = np.concatenate([near, far], 1)
    points = np.concatenate([xyz, rng.random((frames, pts, 3))], -1).astype(np.float32)
    return points.reshape(-1, 6), boxes.reshape(-1, 7)


def crop_loop(points, boxes, frames, pts, nb):
    """per box: mask and index on the device, as the reference's pc[inbox_inds == 0]"""
    out = []
    for f in range(frames):
        pc = points[f * pts:(f + 1) * pts]
        for b in boxes[f * nb:(f + 1) * nb]:
            rot = b[6] + np.pi / 2
            ca, sa = torch.cos(rot), torch.sin(rot)
            dx, dy = pc[:, 0] - b[0], pc[:, 1] - b[1]
            lx, ly = dx * ca - dy * sa, dx * sa + dy * ca
            m = ((pc[:, 2] - (b[2] + b[5] / 2)).abs() <= b[5] / 2) & (lx > -b[4] / 2) & (lx < b[4] / 2) & (ly > -b[3] / 2) & (ly < b[3] / 2)
            out.append(torch.nonzero(m).squeeze(1))
    return out


def timed(fn, repeat):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return dict(median_ms=1e3 * float(np.median(ts)), min_ms=1e3 * min(ts), max_ms=1e3 * max(ts), runs=repeat)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='all', choices=['crop', 'iou', 'all'])
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--loops', type=int, default=1)
    a = ap.parse_args(argv)
    from objectcentricocccompletion_amd import ctrl_prep as cp
    from objectcentricocccompletion_amd.tracklet import Tracklet
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    res = {}
    if a.what in ('crop', 'all'):
        F, N, NB = 200, 150_000, 40
        points, boxes = crop_case(F, N, NB)
        points, boxes = torch.from_numpy(points).to(dev), torch.from_numpy(boxes).to(dev)
        po, bo = list(range(0, F * N + 1, N)), list(range(0, F * NB + 1, NB))
        res['crop_kernels'] = timed(lambda: cp.crop_frames_packed(points, po, boxes, bo), a.repeat)
        counts, idx = cp.crop_frames_packed(points, po, boxes, bo)
        res['crop_memberships'] = int(counts.sum())
        res['crop_bytes_per_pass'] = dict(xyz=F * N * 12, rows=F * N * 24)
        if a.loops:
            res['crop_loop'] = timed(lambda: crop_loop(points, boxes, F, N, NB), max(1, a.loops))
            ref = crop_loop(points, boxes, F, N, NB)
            got = idx.split(counts.tolist())
            res['crop_loop_differs_on_boxes'] = int(sum(not torch.equal(x, y) for x, y in zip(ref, got)))   # f32 faces only
    if a.what in ('iou', 'all'):
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        from test_gpu_ctrl_prep import iou_scene
        pds, gts = iou_scene(seed=5, P=256, G=128, T=200)
        res['iou_new'] = timed(lambda: cp.segment_candidates(pds, gts, 0.5, dev), a.repeat)
        if a.loops:
            on = lambda trks: [Tracklet(t.boxes.to(dev), t.ts_list) for t in trks]

            def loop():
                dp, dg = on(pds), on(gts)
                out = []
                for p in dp:
                    aff = []
                    for g in dg:
                        ious = p.intersection_ious(g)
                        aff.append(ious.max().item() if ious.numel() else 0)
                    out.append([j for j, v in enumerate(aff) if v > 0.5])
                return out
            res['iou_loop'] = timed(loop, max(1, a.loops))
            res['iou_same_candidates'] = loop() == cp.segment_candidates(pds, gts, 0.5, dev)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
