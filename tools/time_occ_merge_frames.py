#!/usr/bin/env python3
"""The occupancy-enhanced clouds of several sensor frames per online call, timed on the MI355X: F frames merged by ONE
occ_ops.occ_merge_frames call (csrc/occ_merge.hip with a frame table) against F occ_ops.occ_merge calls and against the
operator chain occ_ops.occ_merge_frames_aten (what OCOCC_OCC_MERGE_KERNEL=0 selects), and ONE
TrackletRoIHeadOCC.simple_test_scene_steps_merged call against F simple_test_scene_step(merged=True) calls, in the same run.
    python tools/time_occ_merge_frames.py [--frames 1 4 16] [--points 150000] [--boxes 40] [--inside 500] [--reps 9] [--out FILE.md]
The frames, poses, boxes and slots are those of tools/time_scene_steps.py: a box is a tracklet, a call has --boxes slots and
F rows per slot, slot-major.  "operator": the merge alone, on the cells, flags and row scores one chunked call with
occ=True returned (for the F single calls the same cells regrouped per frame, outside the timed region).  "step": the
whole step of the ococcnet model with random weights on fresh slots (the state is reset outside the timed region).  The
operator forms are checked to give the same bytes, all forms are warmed up, then timed alternately; a measurement is the F
frames between device events and, up to a device synchronise, on the host clock; median (min - max).  A report, not a gate."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_occ_export import fmt, timed   # noqa: E402 (the same measuring functions)
from time_scene_rows import frame        # noqa: E402 (the same synthetic frame)
from time_scene_steps import ego_pose    # noqa: E402 (the same poses)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, nargs='+', default=[1, 4, 16])
    ap.add_argument('--points', type=int, default=150000)
    ap.add_argument('--boxes', type=int, default=40)
    ap.add_argument('--inside', type=int, default=500, help='points inside every box')
    ap.add_argument('--reps', type=int, default=9)
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
    n = args.boxes
    state = rh.online_begin(n, dev, cap=max(args.frames))
    labels = torch.zeros(n, dtype=torch.long, device=dev)
    dim = (0, 1, 2, 3, 4)
    lines = ['| frames | points per frame | boxes per frame | cells / survivors | what | form | device events, ms: median (min - max) | host clock, ms |',
             '|---|---|---|---|---|---|---|---|']
    with torch.no_grad():
        for F in args.frames:
            per = [frame(args.points, n, args.inside, dev, seed=f) for f in range(F)]       # (cloud, boxes, scores, matrices)
            poses = np.stack([ego_pose(f) for f in range(F)])
            slot_major = [(s, f) for s in range(n) for f in range(F)]
            pick = lambda k: torch.stack([per[f][k][s] for s, f in slot_major])
            points, sizes = torch.cat([p[0] for p in per]), [p[0].size(0) for p in per]
            boxes, scores = pick(1), pick(2)
            frame_rows, slot_rows = [f for _, f in slot_major], [s for s, _ in slot_major]
            labels_rows = torch.zeros(n * F, dtype=torch.long, device=dev)
            state.reset()
            first = rh.simple_test_scene_steps(points, sizes, poses, boxes, scores, labels_rows, frame_rows, slot_rows, state, occ=True)
            state.reset()
            occ, flags, counts = first['occ_ego'], first['occ_flags'], first['occ_counts']
            row_score = torch.where(first['valid'].to(dev).bool(), first['scores'].float(), scores.float())
            cuts = np.cumsum([0] + list(counts))
            single = []                                   # per frame: cloud, cells, counts, scores, flags of its rows
            for f in range(F):
                rows = [i for i, g in enumerate(frame_rows) if g == f]
                cat = lambda t: torch.cat([t[cuts[i]:cuts[i + 1]] for i in rows]).contiguous()
                single.append((per[f][0], cat(occ), [counts[i] for i in rows], row_score[rows].contiguous(), cat(flags)))
            frames_args = (points, sizes, occ, counts, frame_rows, dim)
            forms = {
                ('operator', 'one `occ_merge_frames` call'): lambda: occ_ops.occ_merge_frames(*frames_args, row_score=row_score, flags=flags),
                ('operator', 'F `occ_merge` calls'): lambda: [occ_ops.occ_merge(p, o, c, dim, row_score=s, flags=g) for p, o, c, s, g in single],
                ('operator', 'chain `occ_merge_frames_aten`'): lambda: occ_ops.occ_merge_frames_aten(*frames_args, row_score=row_score, flags=flags),
                ('step', 'one `simple_test_scene_steps_merged` call'): lambda: rh.simple_test_scene_steps_merged(
                    points, sizes, poses, boxes, scores, labels_rows, frame_rows, slot_rows, state),
                ('step', 'F `simple_test_scene_step(merged=True)` calls'): lambda: [rh.simple_test_scene_step(
                    per[f][0], poses[f], per[f][1], per[f][2], labels, list(range(n)), state, merged=True) for f in range(F)],
            }
            ops = [k for k in forms if k[0] == 'operator']
            one, many, chain = (forms[k]() for k in ops)
            assert torch.equal(one[0].view(torch.int32), torch.cat([m[0] for m in many]).view(torch.int32)), 'frames call != F calls'
            assert torch.equal(one[0].view(torch.int32), chain[0].view(torch.int32)) and one[1:] == chain[1:], 'frames call != chain'
            cells = f'{occ.size(0)} / {sum(one[2])}'
            times = {k: ([], []) for k in forms}
            for rep in range(args.warmup + args.reps):        # alternating: drift of the shared host hits all alike
                for k, fn in forms.items():
                    state.reset()
                    e, h = timed(fn, 1)
                    if rep >= args.warmup:
                        times[k][0].extend(e)
                        times[k][1].extend(h)
            state.reset()
            for (what, form), (e, h) in times.items():
                lines.append(f'| {F} | {args.points} | {n} | {cells} | {what} | {form} | {fmt(e)} | {fmt(h)} |')
                print(lines[-1], flush=True)
    text = '\n'.join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
