#!/usr/bin/env python3
"""Several sensor frames per online call, timed on the MI355X: F frames given to ONE scene_rows.scene_steps_rows /
TrackletRoIHeadOCC.simple_test_scene_steps call against the same F frames given to F scene_step_rows /
simple_test_scene_step calls, in the same run.
    python tools/time_scene_steps.py [--frames 1 4 16] [--points 150000] [--boxes 40] [--inside 500] [--reps 9] [--out FILE.md]
Every frame is the synthetic frame of tools/time_scene_rows.py (--points points, --inside of them in each of --boxes boxes,
the rest background) under its own ego pose; a box is a tracklet, so a call has --boxes slots and F rows per slot,
slot-major.  "operator": the rows alone, with a rigid transform per row, the ococcnet range and max_points 1024.  "step":
the whole step of the ococcnet model with random weights on fresh slots (the state is reset outside the timed region).
Both forms are checked to give the same row counts, warmed up, then timed alternately; a measurement is the F frames
between device events and, up to a device synchronise, on the host clock; median (min - max).  A report, not a gate."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_occ_export import fmt, timed   # noqa: E402 (the same measuring functions)
from time_scene_rows import RANGE, frame   # noqa: E402 (the same synthetic frame)


def ego_pose(f):
    import numpy as np
    a = 0.01 * f
    pose = np.eye(4)
    pose[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    pose[:3, 3] = [1.5 * f, 0.05 * f * f, 0.0]
    return pose


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, nargs='+', default=[1, 4, 16])
    ap.add_argument('--points', type=int, default=150000)
    ap.add_argument('--boxes', type=int, default=40)
    ap.add_argument('--inside', type=int, default=500, help='points inside every box')
    ap.add_argument('--max-points', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the table to this markdown file')
    args = ap.parse_args()
    import numpy as np
    import torch
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (registers)
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    from objectcentricocccompletion_amd.scene_rows import scene_step_rows, scene_steps_rows
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is nothing to time without one'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    rh = DETECTORS.build(ococcnet_model_cfg()).to(dev).eval().roi_head
    n = args.boxes
    state = rh.online_begin(n, dev, cap=max(args.frames))
    labels = torch.zeros(n, dtype=torch.long, device=dev)
    kw = dict(extra_width=1.0, attr_dims=2, point_cloud_range=RANGE, max_points=args.max_points)
    lines = ['| frames | points per frame | boxes per frame | rows | what | form | device events, ms: median (min - max) | host clock, ms |',
             '|---|---|---|---|---|---|---|---|']
    for F in args.frames:
        per = [frame(args.points, n, args.inside, dev, seed=f) for f in range(F)]       # (cloud, boxes, scores, matrices)
        poses = np.stack([ego_pose(f) for f in range(F)])
        slot_major = [(s, f) for s in range(n) for f in range(F)]
        pick = lambda k: torch.stack([per[f][k][s] for s, f in slot_major])
        points, sizes = torch.cat([p[0] for p in per]), [p[0].size(0) for p in per]
        boxes, scores, mats = pick(1), pick(2), pick(3)
        frame_rows, slot_rows = [f for _, f in slot_major], [s for s, _ in slot_major]
        labels_rows = torch.zeros(n * F, dtype=torch.long, device=dev)
        forms = {
            ('operator', 'one frames call'): lambda: scene_steps_rows(points, sizes, boxes, scores, frame_rows, transforms=mats, **kw),
            ('operator', 'F single calls'): lambda: [scene_step_rows(p[0], p[1], p[2], transforms=p[3], **kw) for p in per],
            ('step', 'one frames call'): lambda: rh.simple_test_scene_steps(points, sizes, poses, boxes, scores, labels_rows, frame_rows,
                                                                            slot_rows, state),
            ('step', 'F single calls'): lambda: [rh.simple_test_scene_step(per[f][0], poses[f], per[f][1], per[f][2], labels,
                                                                           list(range(n)), state) for f in range(F)],
        }
        one, many = forms[('operator', 'one frames call')](), forms[('operator', 'F single calls')]()
        rows = one[0].size(0)
        assert rows == sum(m[0].size(0) for m in many) and int(one[3].sum()) == sum(int(m[3].sum()) for m in many), \
            'the two forms disagree on the rows'
        times = {k: ([], []) for k in forms}
        for rep in range(args.warmup + args.reps):        # alternating: drift of the shared host hits both alike
            for k, fn in forms.items():
                state.reset()
                e, h = timed(fn, 1)
                if rep >= args.warmup:
                    times[k][0].extend(e)
                    times[k][1].extend(h)
        state.reset()
        for (what, form), (e, h) in times.items():
            lines.append(f'| {F} | {args.points} | {n} | {rows} | {what} | {form} | {fmt(e)} | {fmt(h)} |')
            print(lines[-1], flush=True)
    text = '\n'.join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
