#!/usr/bin/env python3
"""One frame of online inference, timed on the MI355X: TrackletRoIHeadOCC.simple_test_step (one new frame per tracklet over
the temporal K/V cache) at frame t = 1, 50 and 199 for 1 and 64 tracklets at a time on the ococcnet model, against what a
user without it does at that frame: TrackletRoIHeadOCC.simple_test on the prefix of t + 1 frames, once per tracklet
(simple_test takes one tracklet per call).
    python tools/time_online.py [--slots 1 64] [--frames 1 50 199] [--long-frame 1000] [--catch-up 32] [--points 256]
                                [--reps 7] [--out FILE.md]
Synthetic vehicle tracklets (oracle/synth.py) of --points points per frame, random weights.  For a step at frame t the
cache is set to t cached frames of random keys and values -- what it holds does not change the work -- and pos is set back
after every call.  Both paths are warmed up at every shape, then timed alternately; a call is timed with device events
around it and with the host clock up to a device synchronise; median (min - max) of the repetitions.  A report, not a gate.

Past 256 frames (--long-frame, default 1000; 0: skip): two more rows per tracklet count, a step at that frame of a ring cache
of 16 rows with test_cfg.attn_window_size = 16 and of a long cache of --long-frame + 1 rows without a window (the step
reads 16 and --long-frame cached frames).  The points and boxes are those of the last synthetic frame -- only the frame
index the positional encoding gets and the cache counter say 1000 -- so no longer synthetic tracklets are built.

Several frames per call (--catch-up, default 32; 0: skip): three more rows per tracklet count, bringing every tracklet from
frame 0 to frame --catch-up of a reset cache -- by that many simple_test_step calls, by simple_test_steps calls of 8 frames
per tracklet, and by one simple_test_steps call with all frames.  The inputs of every call are prepared beforehand; the
three forms are warmed up, then timed alternately; the last column divides the median of the device events by the frames."""
import argparse
import os

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')  # before the HIP runtime loads: objectcentricocccompletion_amd/graph.py
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_occ_export import fmt, timed   # noqa: E402 (the same measuring functions)


def tracklets(slots, frames, points, dev, seed=0):
    """per tracklet: boxes [T, 7], scores [T], and its decorated points [n, 3 + 7] with their frame index"""
    import numpy as np
    import torch
    from oracle import synth
    t = synth.synth_tracklets(slots, frames, points, seed=seed)
    rng = np.random.default_rng(seed)
    out = []
    for b in range(slots):
        rb = t['rois'][t['rois'][:, 0] == b][:, 1:]
        m = t['pts_batch'] == b
        score = rng.uniform(0.3, 1.0, size=frames).astype(np.float32)
        fr = t['pts_frame'][m]
        deco = np.concatenate([t['pts_attr'][m], rb[fr][:, 6:7] / np.pi, rb[fr][:, 3:6] / 10, score[fr][:, None]], 1)
        pts = np.concatenate([t['pts_xyz'][m], deco], 1).astype(np.float32)
        order = np.argsort(fr, kind='stable')
        out.append(dict(boxes=torch.from_numpy(rb).to(dev), scores=torch.from_numpy(score).to(dev),
                        points=torch.from_numpy(pts[order]).to(dev), frame=torch.from_numpy(fr[order]).to(dev),
                        ends=np.searchsorted(fr[order], np.arange(frames), side='right')))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--slots', type=int, nargs='+', default=[1, 64])
    ap.add_argument('--frames', type=int, nargs='*', default=[1, 50, 199])
    ap.add_argument('--points', type=int, default=256, help='points per frame and tracklet')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--long-frame', type=int, default=1000, help='frame of the ring / long cache rows (0: none)')
    ap.add_argument('--catch-up', type=int, default=32, help='frames of the several-frames-per-call rows (0: none)')
    ap.add_argument('--out', default=None, help='also write the table to this markdown file')
    args = ap.parse_args()
    import torch
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (registers)
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    from objectcentricocccompletion_amd.tracklet import Tracklet
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is nothing to time without one'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    cfg = ococcnet_model_cfg()
    cfg['test_cfg']['test_occ_iou'] = False          # (no labels here: the refinement alone, on both sides)
    rh = DETECTORS.build(cfg).to(dev).eval().roi_head
    total = max(max(args.frames, default=1) + 1, args.catch_up)
    chunk_lines = ['| tracklets | frames | path | calls | device events, ms: median (min - max) | host clock, ms | '
                   'per frame, ms |', '|---|---|---|---|---|---|---|']
    lines = ['| tracklets | frame t | path | device events, ms: median (min - max) | host clock, ms |', '|---|---|---|---|---|']
    with torch.no_grad():
        for slots in args.slots:
            trks = tracklets(slots, total, args.points, dev)
            state = rh.online_begin(slots, dev)
            for k, v in zip(state.cache.k, state.cache.v):
                k.normal_()
                v.normal_()
            labels = torch.zeros(slots, dtype=torch.long, device=dev)
            slot = list(range(slots))

            def frame_inputs(t):
                lo = [0 if t == 0 else int(d['ends'][t - 1]) for d in trks]
                pts = torch.cat([d['points'][a:int(d['ends'][t])] for d, a in zip(trks, lo)])
                batch = torch.cat([torch.full((int(d['ends'][t]) - a,), b, dtype=torch.long, device=dev)
                                   for b, (d, a) in enumerate(zip(trks, lo))])
                boxes = torch.stack([d['boxes'][t] for d in trks])
                scores = torch.stack([d['scores'][t] for d in trks])
                return pts[:, :3].contiguous(), pts[:, 3:].contiguous(), batch, boxes, scores

            for t in args.frames:
                xyz, feats, batch, boxes, scores = frame_inputs(t)

                def step():
                    state.cache.pos.fill_(t)
                    state.cache.pos_host[:] = [t] * slots
                    return rh.simple_test_step(xyz, feats, batch, boxes, scores, labels, slot, state)

                prefixes = []
                for d in trks:
                    n = int(d['ends'][t])
                    p = d['points'][:n]
                    prefixes.append((p[:, :3].contiguous(), p[:, 3:].contiguous(), torch.zeros(n, dtype=torch.long, device=dev),
                                     d['frame'][:n], Tracklet(d['boxes'][:t + 1], list(range(t + 1)), d['scores'][:t + 1], type=0)))

                def offline():
                    for x, f, b, fr, trk in prefixes:
                        rh.simple_test(x, f, b, fr, None, [trk])

                for _ in range(args.warmup):
                    step()
                    offline()
                times = {'step': ([], []), 'offline': ([], [])}
                for _ in range(args.reps):            # alternating: drift of the shared host hits both alike
                    for name, fn in (('step', step), ('offline', offline)):
                        e, h = timed(fn, 1)
                        times[name][0].extend(e)
                        times[name][1].extend(h)
                for name, what in (('step', '`simple_test_step`, one launch set for all tracklets'),
                                   ('offline', f'`simple_test` on frames 0..{t}, once per tracklet')):
                    lines.append(f'| {slots} | {t} | {what} | {fmt(times[name][0])} | {fmt(times[name][1])} |')
                    print(lines[-1], flush=True)
            if args.catch_up > 0:
                F = args.catch_up

                def chunk_inputs(a, T):
                    """the frames a..a+T-1 of every tracklet as rows b * T + (t - a): the rows of a slot consecutive"""
                    lo = [0 if a == 0 else int(d['ends'][a - 1]) for d in trks]
                    hi = [int(d['ends'][a + T - 1]) for d in trks]
                    pts = torch.cat([d['points'][x:y] for d, x, y in zip(trks, lo, hi)])
                    row = torch.cat([d['frame'][x:y].long() - a + b * T for b, (d, x, y) in enumerate(zip(trks, lo, hi))])
                    return (pts[:, :3].contiguous(), pts[:, 3:].contiguous(), row, torch.cat([d['boxes'][a:a + T] for d in trks]),
                            torch.cat([d['scores'][a:a + T] for d in trks]), torch.zeros(slots * T, dtype=torch.long, device=dev),
                            [b for b in range(slots) for _ in range(T)])

                single = [frame_inputs(t) for t in range(F)]
                forms = [('step', f'{F} `simple_test_step` calls', F, None)]
                for T in dict.fromkeys((min(8, F), F)):
                    calls = [chunk_inputs(a, min(T, F - a)) for a in range(0, F, T)]
                    forms.append((f'chunk{T}', f'`simple_test_steps`, {T} frames per tracklet and call', len(calls), calls))

                def catch_up(calls):
                    state.reset()
                    if calls is None:
                        for xyz, feats, batch, boxes, scores in single:
                            rh.simple_test_step(xyz, feats, batch, boxes, scores, labels, slot, state)
                    else:
                        for xyz, feats, row, boxes, scores, lab, slot_rows in calls:
                            rh.simple_test_steps(xyz, feats, row, boxes, scores, lab, slot_rows, state)
                    assert state.frames == [F] * slots

                for _ in range(args.warmup):
                    for _, _, _, calls in forms:
                        catch_up(calls)
                times = {name: ([], []) for name, _, _, _ in forms}
                for _ in range(args.reps):            # alternating, as above
                    for name, _, _, calls in forms:
                        e, h = timed(lambda: catch_up(calls), 1)
                        times[name][0].extend(e)
                        times[name][1].extend(h)
                for name, what, ncalls, _ in forms:
                    e, h = times[name]
                    chunk_lines.append(f'| {slots} | {F} | {what} | {ncalls} | {fmt(e)} | {fmt(h)} | '
                                       f'{sorted(e)[len(e) // 2] / F:.3f} |')
                    print(chunk_lines[-1], flush=True)
            del state
            if args.long_frame > 0:
                T = args.long_frame
                xyz, feats, batch, boxes, scores = frame_inputs(total - 1)
                cfgs = list({id(c): c for c in (rh.test_cfg, rh.bbox_head.test_cfg)}.values())
                for what, kw, window in ((f'`simple_test_step`, ring cache of 16 rows, window 16', dict(cap=16, ring=True), 16),
                                         (f'`simple_test_step`, long cache of {T + 1} rows, no window', dict(cap=T + 1, long=True),
                                          -1)):
                    st = rh.online_begin(slots, dev, **kw)
                    for k, v in zip(st.cache.k, st.cache.v):
                        k.normal_()
                        v.normal_()
                    for c in cfgs:
                        c['attn_window_size'] = window

                    def step_long():
                        st.cache.pos.fill_(T)
                        st.cache.pos_host[:] = [T] * slots
                        return rh.simple_test_step(xyz, feats, batch, boxes, scores, labels, slot, st)

                    try:
                        for _ in range(args.warmup):
                            step_long()
                        e, h = timed(step_long, args.reps)
                    finally:
                        for c in cfgs:
                            del c['attn_window_size']
                    lines.append(f'| {slots} | {T} | {what} | {fmt(e)} | {fmt(h)} |')
                    print(lines[-1], flush=True)
                    del st
    text = '\n'.join(lines)
    if len(chunk_lines) > 2:
        text += '\n\n' + '\n'.join(chunk_lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
