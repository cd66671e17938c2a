#!/usr/bin/env python
"""Time waymo_metrics.detection_metrics on a synthetic input of validation-split size and print one JSON line:
host packing, kernels (uploads, the launches, the read-back) and host curves, each over --repeats runs after --warmup.

    python tools/time_waymo_metrics.py [--frames 40000] [--gt 60] [--pred 80] [--repeats 5] [--warmup 1] [--checker-frames 0]
                                        [--matcher {score_first,hungarian}]

--checker-frames N additionally times the float64 checker of the tests (tests/waymo_metrics_ref.py) on the first N
frames, for scale.  The input is drawn from a seed: ground truth spread over +-75 m, three of four predictions
perturbed copies of a ground-truth box."""
import argparse
import json
import os
import resource
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_columns(frames, n_gt, n_pd, seed=0):
    rng = np.random.default_rng(seed)
    G, P = frames * n_gt, frames * n_pd
    t = rng.choice([1, 1, 1, 2, 2, 4, 3], G)
    lo = np.array([[0, 0, 0], [3.5, 1.6, 1.4], [0.5, 0.5, 1.4], [0.3, 0.1, 0.5], [1.4, 0.5, 1.4]])
    hi = np.array([[1, 1, 1], [6.0, 2.4, 2.2], [1.1, 1.0, 2.0], [0.9, 0.4, 1.2], [2.1, 0.9, 1.9]])
    gb = np.empty((G, 7))
    gb[:, :2] = rng.uniform(-75, 75, (G, 2))
    gb[:, 2] = rng.uniform(-1, 2, G)
    gb[:, 3:6] = lo[t] + rng.random((G, 3)) * (hi[t] - lo[t])
    gb[:, 6] = rng.uniform(-np.pi, np.pi, G)
    frame_g = np.repeat(np.arange(frames), n_gt)
    src = (np.repeat(np.arange(frames), n_pd) * n_gt + rng.integers(0, n_gt, P))      # a ground-truth box of the same frame
    pb, pt = gb[src].copy(), t[src].copy()
    s = rng.choice([0.01, 0.03, 0.08, 0.2], P)[:, None]
    pb[:, :3] += rng.normal(0, 1, (P, 3)) * s * np.stack([pb[:, 3], pb[:, 4], np.full(P, 0.5)], 1)
    pb[:, 3:6] *= 1 + rng.normal(0, 1, (P, 3)) * s / 2
    pb[:, 6] += rng.normal(0, 1, P) * s[:, 0] / 2
    free = rng.random(P) < 0.25
    pb[free, :2] = rng.uniform(-75, 75, (int(free.sum()), 2))
    frame_p = np.repeat(np.arange(frames), n_pd)
    names = np.array([f'segment-{i:05d}' for i in range((frames + 197) // 198)], dtype=object)
    keys = ('center_x', 'center_y', 'center_z', 'length', 'width', 'height', 'heading')

    def cols(b, ty, fr, score, **extra):
        c = {k: b[:, i].astype(np.float32).astype(np.float64) for i, k in enumerate(keys)}
        c.update(type=ty.astype(np.int64), score=score, context_name=names[fr // 198],
                 frame_timestamp_micros=(fr % 198).astype(np.int64) * 100000 + 1550000000000000, **extra)
        return c

    u = rng.random(G)
    gt = cols(gb, t, frame_g, np.ones(G), detection_difficulty_level=np.where(u < 0.1, 2, 1).astype(np.int64),
              num_lidar_points_in_box=np.where(u < 0.2, 0, np.where(u < 0.35, 3, 40)).astype(np.int64),
              overlap_with_nlz=np.zeros(G, bool))
    pd = cols(pb, pt, frame_p, rng.uniform(0.02, 1.0, P).astype(np.float32).astype(np.float64), overlap_with_nlz=rng.random(P) < 0.05)
    return pd, gt


def records(c, n):
    return [{k: (v[i].item() if hasattr(v[i], 'item') else v[i]) for k, v in c.items()} for i in range(n)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=40000)
    ap.add_argument('--gt', type=int, default=60)
    ap.add_argument('--pred', type=int, default=80)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--checker-frames', type=int, default=0)
    ap.add_argument('--matcher', choices=('score_first', 'hungarian'), default='score_first')
    a = ap.parse_args(argv)
    import torch
    from objectcentricocccompletion_amd import waymo_metrics as M
    assert torch.cuda.is_available(), 'timing needs the GPU'
    pd, gt = synthetic_columns(a.frames, a.gt, a.pred)
    runs, ap_dict = [], None
    for r in range(a.warmup + a.repeats):
        t = {}
        t0 = time.perf_counter()
        _, ap_dict = M.detection_metrics(pd, gt, timings=t, matcher=a.matcher)
        t['total'] = time.perf_counter() - t0
        if r >= a.warmup:
            runs.append(t)
    # the device part alone: events around frame_match (frame_assign with --matcher hungarian) on resident tensors
    pk = M.pack(pd, gt)
    dev = torch.device('cuda', torch.cuda.current_device())
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x.astype(dt))).to(dev)
    args = (up(pk['pd_boxes'], np.float32), up(pk['pd_type'], np.int32), up(pk['pd_eligible'], np.int32), pk['pd_offsets'],
            up(pk['gt_boxes'], np.float32), up(pk['gt_type'], np.int32), up(pk['gt_eligible'], np.int32), pk['gt_offsets'])
    if a.matcher == 'hungarian':
        # the snapshot layout is host arithmetic on the scores: made once, outside the events
        layout = M.snapshot_layout(pk['pd_offsets'], pk['pd_type'], M.cutoff_buckets(pk['pd_score']))
        device_part = lambda: M.frame_assign(*args, layout=layout)
    else:
        device_part = lambda: M.frame_match(*args)
    dev_ms = []
    for r in range(a.warmup + a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        device_part()
        e1.record()
        torch.cuda.synchronize()
        if r >= a.warmup:
            dev_ms.append(e0.elapsed_time(e1))
    stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
    n_rec = min(len(pd['score']), 200000)
    t0 = time.perf_counter()
    recs = records(pd, n_rec)
    t1 = time.perf_counter()
    M.columns(recs)
    t2 = time.perf_counter()
    out = dict(matcher=a.matcher, frames=a.frames, predictions=len(pd['score']), ground_truth=len(gt['score']),
               pairs=int(a.frames) * a.gt * a.pred, repeats=a.repeats,
               seconds={k: stat([t[k] for t in runs]) for k in ('host_pack', 'kernels', 'host_curves', 'total')},
               columns_from_records_us_per_object=(t2 - t1) / n_rec * 1e6,
               vehicle_l1_map=ap_dict['Vehicle/L1 mAP'])
    # between events, tensors resident: frame_match, or frame_assign with its snapshot buffer (allocated and filled inside)
    out['frame_match_device_ms' if a.matcher == 'score_first' else 'frame_assign_device_ms'] = stat(dev_ms)
    if a.matcher == 'hungarian':
        out['snapshot_words'] = int(layout['total'])
        out['snapshots'] = int(len(layout['ends']))
    out['peak_rss_mb'] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0
    if a.checker_frames:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import waymo_metrics_ref as R
        p = records(pd, a.checker_frames * a.pred)
        g = records(gt, a.checker_frames * a.gt)
        t0 = time.perf_counter()
        m = R.match(p, g)
        t1 = time.perf_counter()
        R.table(p, g, m)
        t2 = time.perf_counter()
        out['checker'] = dict(frames=a.checker_frames, match_seconds=t1 - t0, curves_seconds=t2 - t1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
