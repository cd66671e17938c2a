#!/usr/bin/env python3
"""The occupancy-enhanced cloud of one online frame, timed on the MI355X: TrackletRoIHeadOCC.simple_test_scene_step with
``merged=True`` next to ``occ=True`` on the ococcnet model, and occ_ops.occ_merge (csrc/occ_merge.hip) alone next to the
operator chain occ_ops.occ_merge_aten (what OCOCC_OCC_MERGE_KERNEL=0 selects) on the step's own cells, for 1, 16 and 64
tracklets at a time over a synthetic scene cloud of --cloud points.
    python tools/time_occ_merge.py [--slots 1 16 64] [--cloud 180000] [--points 256] [--reps 7] [--out FILE.md]
The tracklets are those of tools/time_online.py (their first frame; every call steps a reset state), the measuring
functions those of tools/time_occ_export.py.  All forms run in ONE process: warmed up at every shape, then timed
alternately, --reps times each, with device events around a call and with the host clock up to a device synchronise;
median (min - max).  Per form also the device launches of one call (kernels + copies / memsets, from torch's profiler).
A report, not a gate."""
import argparse
import os

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')  # before the HIP runtime loads: objectcentricocccompletion_amd/graph.py
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_occ_export import count_launches, fmt, timed   # noqa: E402 (the same measuring functions)
from time_online import tracklets                        # noqa: E402 (the same synthetic tracklets)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--slots', type=int, nargs='+', default=[1, 16, 64])
    ap.add_argument('--cloud', type=int, default=180000, help='background points of the scene cloud')
    ap.add_argument('--points', type=int, default=256, help='points per tracklet in the frame')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the table to this markdown file')
    args = ap.parse_args()
    import numpy as np
    import torch
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (registers)
    from objectcentricocccompletion_amd.occ import occ_ops
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is nothing to time without one'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    cfg = ococcnet_model_cfg()
    cfg['test_cfg']['test_occ_iou'] = False
    rh = DETECTORS.build(cfg).to(dev).eval().roi_head
    lines = ['| tracklets | form | device events, ms: median (min - max) | host clock, ms | launches: kernels + copies | '
             'cloud rows + cells / survivors |', '|---|---|---|---|---|---|']

    def shape(slots):
        trks = tracklets(slots, 2, args.points, dev)
        g = torch.Generator().manual_seed(slots)
        back = torch.cat([torch.rand(args.cloud, 2, generator=g) * 300 - 150, torch.rand(args.cloud, 1, generator=g) * 4 - 2,
                          torch.rand(args.cloud, 2, generator=g)], 1).to(dev)
        own = torch.cat([d['points'][:int(d['ends'][0]), :5] for d in trks])
        points = torch.cat([back, own])[torch.randperm(args.cloud + own.size(0), generator=g).to(dev)].contiguous()
        boxes, scores = torch.stack([d['boxes'][0] for d in trks]), torch.stack([d['scores'][0] for d in trks])
        labels = torch.zeros(slots, dtype=torch.long, device=dev)
        state = rh.online_begin(slots, dev, cap=4)
        slot, pose = list(range(slots)), np.eye(4)

        def step(**kw):
            state.reset()
            return rh.simple_test_scene_step(points, pose, boxes, scores, labels, slot, state, **kw)

        first = step(merged=True)
        occ, flags, counts = first['occ_ego'], first['occ_flags'], first['occ_counts']
        row_score = torch.where(first['valid'].to(dev).bool(), first['scores'].float(), scores.float())
        op = lambda f: f(points, occ, counts, (0, 1, 2, 3, 4), row_score=row_score, flags=flags)
        forms = [('occ', '`simple_test_scene_step(occ=True)`', lambda: step(occ=True)),
                 ('merged', '`simple_test_scene_step(merged=True)`, `csrc/occ_merge.hip`', lambda: step(merged=True)),
                 ('kernel', '`occ_ops.occ_merge` alone', lambda: op(occ_ops.occ_merge)),
                 ('chain', '`occ_ops.occ_merge_aten` alone (`OCOCC_OCC_MERGE_KERNEL=0`)', lambda: op(occ_ops.occ_merge_aten))]
        return forms, f'{points.size(0)} + {occ.size(0)} / {sum(first["merged_counts"])}'

    with torch.no_grad():
        shapes = []
        for slots in args.slots:                      # the end-to-end figures first, the profiler off
            forms, rows = shape(slots)
            for _ in range(args.warmup):
                for _, _, fn in forms:
                    fn()
            times = {name: ([], []) for name, _, _ in forms}
            for _ in range(args.reps):                # alternating: drift of the shared host hits all alike
                for name, _, fn in forms:
                    e, h = timed(fn, 1)
                    times[name][0].extend(e)
                    times[name][1].extend(h)
            shapes.append((slots, forms, rows, times))
        for slots, forms, rows, times in shapes:      # then the launches of one call each, under the profiler
            for name, what, fn in forms:
                kernels, copies = count_launches(fn)
                e, h = times[name]
                lines.append(f'| {slots} | {what} | {fmt(e)} | {fmt(h)} | {kernels} + {copies} | {rows} |')
                print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
