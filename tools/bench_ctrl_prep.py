"""Timing of the tracklet data preparation kernels against the per-box / per-pair loops they replace
(profiles/ctrl_prep.md).  Needs the MI355X; no fallback.

  python tools/bench_ctrl_prep.py [--what crop|iou|nonempty|extend|all] [--repeat 5] [--loops 1]

crop: 200 frames x 150 000 points x 40 enlarged boxes, ctrl_prep.crop_frames_packed against, per box, a torch mask and
      nonzero on the device (the reference's loop, generate_track_input.py:84-99, minus its per-box copies).
iou:  P = 256 predicted, G = 128 GT tracklets over 200 frames, ctrl_prep.segment_candidates against a Python loop of
      Tracklet.intersection_ious(...).max().item() per pair (generate_candidates.py:61-65).
nonempty: the crop batch again, ctrl_prep.nonempty_frames_packed (flags only) beside the count launch alone
      (ococc_tracklet_crop_count, no read-back, no fill) and beside crop_frames_packed(...)[0] > 0.
extend: 1 000 tracklets over 8 segments of 200 frames, one ctrl_prep.extend_tracks_packed launch (upload of the tables
      included) against the per-tracklet host loop of Tracklet.frame_transform / shared2ego on CPU tensors, which is
      where the reference's tools/ctrl/extend_tracks.py runs its loop (and which leaves out its extend step).
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


def extend_case(segments=8, frames=200, tracklets=1000, seed=2):
    rng = np.random.default_rng(seed)
    poses = np.tile(np.eye(4, dtype=np.float32), (segments * frames, 1, 1))
    ang = 0.01 * np.arange(segments * frames)
    poses[:, 0, 0], poses[:, 0, 1], poses[:, 1, 0], poses[:, 1, 1] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)
    poses[:, :3, 3] = np.stack([2000 + 1.5 * np.arange(segments * frames), -3000 + 0.2 * np.arange(segments * frames), np.zeros(segments * frames)], 1)
    stamps = np.concatenate([1_000_000_000 * (s + 1) + 100_000 * np.arange(frames) for s in range(segments)]).astype(np.int64)
    offsets, fr, seg = [0], [], []
    for t in range(tracklets):
        lo = int(rng.integers(0, frames - 20))
        hi = int(rng.integers(lo + 5, min(frames, lo + 120)))
        fr += list(range(lo, hi))
        offsets.append(len(fr))
        seg.append(t % segments)
    n = len(fr)
    boxes = np.concatenate([rng.uniform(-50, 50, (n, 2)), rng.uniform(-1, 1, (n, 1)), rng.uniform(1.5, 5, (n, 3)), rng.uniform(-3, 3, (n, 1))], 1)
    return dict(boxes=boxes.astype(np.float32), scores=rng.uniform(0.1, 1, n), offsets=np.asarray(offsets), frames=np.asarray(fr),
                segments=np.asarray(seg), poses=poses.reshape(-1, 16), timestamps=stamps,
                seg_offsets=np.arange(segments + 1) * frames)


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
    ap.add_argument('--what', default='all', choices=['crop', 'iou', 'nonempty', 'extend', 'all'])
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
    if a.what in ('nonempty', 'all'):
        from objectcentricocccompletion_amd import _lib as L
        F, N, NB = 200, 150_000, 40
        points, boxes = crop_case(F, N, NB)
        points, boxes = torch.from_numpy(points).to(dev), torch.from_numpy(boxes).to(dev)
        po, bo = list(range(0, F * N + 1, N)), list(range(0, F * NB + 1, NB))
        offs = torch.tensor(po + bo, dtype=torch.int64).to(dev)
        counts = torch.zeros(F * NB, dtype=torch.int64, device=dev)
        ws_bytes = (N + 4095) // 4096 * 4 * F * NB * 4
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        flags = torch.zeros(F * NB, dtype=torch.int32, device=dev)
        count_only = lambda: L.check(L.lib.ococc_tracklet_crop_count(
            L.ptr(points), F * N, 6, L.ptr(offs[:F + 1]), L.ptr(boxes), F * NB, L.ptr(offs[F + 1:]), F, N, L.ptr(counts), L.ptr(ws),
            ws_bytes, L.stream()), 'count')
        flags_only = lambda: L.check(L.lib.ococc_tracklet_nonempty(
            L.ptr(points), F * N, 6, L.ptr(offs[:F + 1]), L.ptr(boxes), F * NB, L.ptr(offs[F + 1:]), F, N, L.ptr(flags), L.stream()), 'flags')
        res['count_launch'] = timed(count_only, a.repeat)
        res['nonempty_launch'] = timed(flags_only, a.repeat)
        res['nonempty_op'] = timed(lambda: cp.nonempty_frames_packed(points, po, boxes, bo).cpu(), a.repeat)
        res['crop_gt0_op'] = timed(lambda: cp.crop_frames_packed(points, po, boxes, bo)[0] > 0, a.repeat)
        res['nonempty_same_flags'] = bool(torch.equal(flags.cpu() > 0, counts.cpu() > 0))
        res['nonempty_boxes'] = int(flags.sum())
    if a.what in ('extend', 'all'):
        fx = extend_case()
        seg_ts = [fx['timestamps'][x:y].tolist() for x, y in zip(fx['seg_offsets'], fx['seg_offsets'][1:])]
        plan = cp.plan_extension(fx['offsets'], fx['frames'], fx['segments'], seg_ts, 10, 3)
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
        d = {k: up(fx[k]) for k in ('boxes', 'scores', 'poses', 'timestamps')}
        run = lambda: cp.extend_tracks_packed(d['boxes'], fx['offsets'], fx['frames'], fx['segments'], d['scores'], d['poses'],
                                              d['timestamps'], fx['seg_offsets'], *plan, 0.9, 10)
        res['extend_kernel'] = timed(run, a.repeat)
        res['extend_boxes'] = dict(input=int(fx['offsets'][-1]), output=int(plan[2][-1]), tracklets=len(fx['segments']))
        if a.loops:
            poses = torch.from_numpy(fx['poses'].reshape(-1, 4, 4))

            def loop():
                out = []
                for t in range(len(fx['segments'])):
                    lo, hi = fx['offsets'][t], fx['offsets'][t + 1]
                    rows = fx['seg_offsets'][fx['segments'][t]] + fx['frames'][lo:hi]
                    trk = Tracklet(torch.from_numpy(fx['boxes'][lo:hi]), fx['timestamps'][rows].tolist())
                    trk.pose_list = list(poses[rows])
                    trk.frame_transform(trk.pose_list[0])
                    out.append(trk.shared2ego())
                return out
            t0 = time.perf_counter()
            loop()
            res['extend_host_loop'] = dict(median_ms=1e3 * (time.perf_counter() - t0), runs=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
