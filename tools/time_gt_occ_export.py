#!/usr/bin/env python3
"""Crop of the ground-truth occupancy for its export, timed on the MI355X: bbox.crop_gt_occ_aten (the operator chain of the
reference's save_gt_occ branch, a boolean index per frame) against bbox.crop_gt_occ_packed (csrc/gt_occ_crop.hip) on the
same cells and boxes, 8 and 200 frames of 2 500 cells.
    python tools/time_gt_occ_export.py [--frames 8 200] [--cells 2500] [--reps 9] [--out profiles/gt_occ_export.md]
Per size: both paths are warmed up, checked to give the same bytes, then timed alternately; a call is timed with device
events around it and with the host clock (both calls end in a read-back, i.e. are synchronous); the median, minimum and
maximum of the repetitions are reported.  Kernel launches per call come from a torch.profiler run of its own, host
synchronisations from torch's sync-debug warnings."""
import argparse
import math
import os

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')  # before the HIP runtime loads: objectcentricocccompletion_amd/graph.py
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_occ_export import count_launches, count_syncs, fmt, timed   # noqa: E402 (the same measuring functions)


def case(n, k, dev, seed=0):
    """n vehicle-sized GT boxes within 80 m at any yaw, proposals around them, k label cells a little beyond the box"""
    import torch
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    size = torch.tensor([2.0, 4.6, 1.7]) + u(n, 3) * torch.tensor([0.4, 1.0, 0.4])
    gt = torch.cat([u(n, 2) * 80, u(n, 1) * 4, size, u(n, 1) * math.pi], 1)
    roi = gt + torch.cat([u(n, 3) * 0.5, u(n, 3) * 0.3, u(n, 1) * 0.3], 1)
    cells = u(k, 3) * torch.tensor([1.4, 2.9, 1.1])
    return cells.to(dev), gt.to(dev), roi.to(dev)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, nargs='+', default=[8, 200])
    ap.add_argument('--cells', type=int, default=2500)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the table to this markdown file')
    args = ap.parse_args()
    import torch
    from objectcentricocccompletion_amd import bbox
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is nothing to time without one'
    assert bbox.GT_OCC_KERNEL, 'OCOCC_GT_OCC_KERNEL=0: both paths would be the ATen chain'
    dev = torch.device('cuda:0')
    lines = ['| frames | cells | kept | path | device events, ms: median (min - max) | host clock, ms | kernel launches '
             '| copies / memsets | host synchronisations |', '|---|---|---|---|---|---|---|---|---|']
    paths = ('crop_gt_occ_aten', 'crop_gt_occ_packed')
    for n in args.frames:
        cells, gt, roi = case(n, args.cells, dev)
        # (the comparator as the export would use it: the per-frame lists joined into the one array the writer takes)
        old = lambda: torch.cat(bbox.crop_gt_occ_aten(cells, gt, roi))
        new = lambda: bbox.crop_gt_occ_packed(cells, gt, roi)
        for _ in range(args.warmup):
            a, (b, counts) = old(), new()
        assert torch.equal(a, b[:, :3]) and sum(counts) == a.size(0), 'the two paths differ'
        t = {name: ([], []) for name in paths}
        for _ in range(args.reps):                       # alternating: drift of the shared host hits both alike
            for name, fn in zip(paths, (old, new)):
                e, h = timed(fn, 1)
                t[name][0].extend(e)
                t[name][1].extend(h)
        for name, fn in zip(paths, (old, new)):
            syncs = count_syncs(fn)
            k, c = count_launches(fn)
            lines.append(f'| {n} | {args.cells} | {int(b.size(0))} | `{name}` | {fmt(t[name][0])} | {fmt(t[name][1])} | {k} | {c} '
                         f'| {syncs} |')
            print(lines[-1], flush=True)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
