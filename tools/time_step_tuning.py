#!/usr/bin/env python3
"""Tuning per online step, timed on the MI355X: (a) the observation sample -- occ_ops.tune_sample on the
kernels of csrc/tune_sample.hip against the operator chain it replaces for the step, OccAutoEncoder.sample_observation(
balance_sample=True, downsample_size=256) plus the ``seen`` filter of OccBBoxHead.online_tuning, on the pooled points of
tests/golden/ococc_head.npz at 1, 16 and 64 RoIs; (b) TrackletRoIHeadOCC.simple_test_step with and without
tune=dict(num_iter=10, downsample_size=256), with and without occ=True, at 1, 16 and 64 tracklets on the ococcnet model
with the bf16 decoder.
    python tools/time_step_tuning.py [--slots 1 16 64] [--frame 50] [--points 256] [--reps 7] [--out FILE.md]
Inputs of (b), cache handling and measuring functions are those of tools/time_online_occ.py.  All forms of a shape run
in ONE process: warmed up, then timed alternately, --reps times each, with device events around a call and with the host
clock up to a device synchronise; median (min - max); the device launches of one call from torch's profiler in a pass of
their own after the timing.  A report, not a gate."""
import argparse
import os

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')  # before the HIP runtime loads: objectcentricocccompletion_amd/graph.py
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from time_occ_export import count_launches, fmt, timed   # noqa: E402 (the same measuring functions)
from time_online import tracklets                        # noqa: E402 (the same synthetic tracklets)

TUNE = dict(num_iter=10, downsample_size=256, balance_sample=True, seed=0)


def measure(forms, reps, warmup, lines, head):
    """forms [(description, call)]: warm up, time alternately, then count the launches; one table row per form"""
    for _ in range(warmup):
        for _, fn in forms:
            fn()
    times = [([], []) for _ in forms]
    for _ in range(reps):                             # alternating: drift of the shared host hits all alike
        for (_, fn), (e, h) in zip(forms, times):
            a, b = timed(fn, 1)
            e.extend(a)
            h.extend(b)
    for (what, fn), (e, h) in zip(forms, times):
        kernels, copies = count_launches(fn)
        lines.append(f'| {head} | {what} | {fmt(e)} | {fmt(h)} | {kernels} + {copies} |')
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--slots', type=int, nargs='+', default=[1, 16, 64])
    ap.add_argument('--frame', type=int, default=50)
    ap.add_argument('--points', type=int, default=256, help='points per frame and tracklet')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the tables to this markdown file')
    args = ap.parse_args()
    import numpy as np
    import torch
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (registers)
    from objectcentricocccompletion_amd.occ import occ_ops
    from objectcentricocccompletion_amd.occ.occ_base import OccDecoder
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    from objectcentricocccompletion_amd.tracklet import host_index
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is nothing to time without one'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    cfg = ococcnet_model_cfg()
    cfg['test_cfg']['test_occ_iou'] = False
    rh = DETECTORS.build(cfg).to(dev).eval().roi_head
    for mod in rh.modules():
        if isinstance(mod, OccDecoder):
            mod.compute_dtype = torch.bfloat16
    bh = rh.bbox_head
    ae = bh.occ_ae_head
    t = args.frame
    head = '| {} | path | device events, ms: median (min - max) | host clock, ms | launches: kernels + copies |'
    lines = ['(a) the sample', '', head.format('RoIs (points, rows)'), '|---|---|---|---|---|']

    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'ococc_head.npz'))
    g_xyz, g_inds = torch.from_numpy(gold['in_local_xyz']).to(dev), torch.from_numpy(gold['in_roi_inds']).to(dev).long()
    g_rois = torch.from_numpy(gold['in_rois']).to(dev)
    with torch.no_grad():
        for n in args.slots:
            n = min(n, g_rois.size(0))
            first = 1 if n < g_rois.size(0) else 0           # (RoI 0 of the file holds no point)
            sel = (g_inds >= first) & (g_inds < first + n)
            xyz, inds, rois = g_xyz[sel].contiguous(), (g_inds[sel] - first).contiguous(), g_rois[first:first + n].contiguous()
            seeds = host_index([occ_ops.tune_row_seed(0, s, t) for s in range(n)], dev)
            keep = torch.zeros(n, dtype=torch.bool, device=dev)
            keep[inds] = True
            turned = ae.observation_xyz(xyz)
            layout = occ_ops.dense_grid_layout(rois[:, 4:7], ae.voxel_size, ae.scale_wlh, ae.offset_wlh)

            def parent():
                smp_xyz, labels, smp_inds = ae.sample_observation(xyz, rois, inds, downsample_size=TUNE['downsample_size'],
                                                                  balance_sample=True)
                seen = torch.zeros(n, dtype=torch.bool, device=dev)
                seen[inds] = True
                k = seen[smp_inds.long()]
                return smp_xyz[k], labels[k], smp_inds[k]

            sample = lambda fn: fn(*layout, ae.voxel_size, turned, inds, seeds, keep, balance=True, cap=TUNE['downsample_size'])
            rows = sum(sample(occ_ops.tune_sample)[4])
            forms = [('`sample_observation(balance_sample=True, downsample_size=256)` + `seen` filter (the offline path)', parent),
                     ('`OccAutoEncoder.step_sample`: layout, turn, `occ_ops.tune_sample`',
                      lambda: ae.step_sample(xyz, rois, inds, seeds, keep, downsample_size=TUNE['downsample_size'])),
                     ('`occ_ops.tune_sample` alone, `csrc/tune_sample.hip`', lambda: sample(occ_ops.tune_sample)),
                     ('`occ_ops.tune_sample_aten` alone (`OCOCC_TUNE_SAMPLE_KERNEL=0`)', lambda: sample(occ_ops.tune_sample_aten))]
            measure(forms, args.reps, args.warmup, lines, f'{n} ({xyz.size(0)}, {rows})')

        lines += ['', '(b) the step', '', head.format('tracklets'), '|---|---|---|---|---|']
        for slots in args.slots:
            trks = tracklets(slots, t + 1, args.points, dev)
            state = rh.online_begin(slots, dev)
            for k, v in zip(state.cache.k, state.cache.v):
                k.normal_()
                v.normal_()
            labels = torch.zeros(slots, dtype=torch.long, device=dev)
            slot = list(range(slots))
            lo = [int(d['ends'][t - 1]) for d in trks]
            pts = torch.cat([d['points'][a:int(d['ends'][t])] for d, a in zip(trks, lo)])
            batch = torch.cat([torch.full((int(d['ends'][t]) - a,), b, dtype=torch.long, device=dev)
                               for b, (d, a) in enumerate(zip(trks, lo))])
            boxes, scores = torch.stack([d['boxes'][t] for d in trks]), torch.stack([d['scores'][t] for d in trks])
            xyz, feats = pts[:, :3].contiguous(), pts[:, 3:].contiguous()

            def step(state=state, xyz=xyz, feats=feats, batch=batch, boxes=boxes, scores=scores, labels=labels, slot=slot,
                     slots=slots, **kw):
                state.cache.pos.fill_(t)
                state.cache.pos_host[:] = [t] * slots
                return rh.simple_test_step(xyz, feats, batch, boxes, scores, labels, slot, state, **kw)

            forms = [('`simple_test_step`', lambda: step()),
                     ('`simple_test_step(tune=dict(num_iter=10, downsample_size=256))`', lambda: step(tune=dict(TUNE))),
                     ('`simple_test_step(occ=True)`', lambda: step(occ=True)),
                     ('`simple_test_step(occ=True, tune=...)`', lambda: step(occ=True, tune=dict(TUNE)))]
            measure(forms, args.reps, args.warmup, lines, str(slots))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
