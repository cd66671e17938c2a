#!/usr/bin/env python3
"""One frame of online inference WITH the completed occupancy, timed on the MI355X: TrackletRoIHeadOCC.simple_test_step(...,
occ=True) at frame --frame for 1, 16 and 64 tracklets at a time on the ococcnet model, on the kernels of csrc/occ_frame.hip
and on the operator chain occ_ops.occ_frame_select_aten (what OCOCC_OCC_FRAME_KERNEL=0 selects), next to the plain step.
    python tools/time_online_occ.py [--slots 1 16 64] [--frame 50] [--points 256] [--reps 7] [--out FILE.md]
Inputs, cache handling and measuring functions are those of tools/time_online.py.  All forms run in ONE process: warmed up
at every shape, then timed alternately, --reps times each, with device events around a call and with the host clock up to
a device synchronise; median (min - max).  Per form also the device launches of one call (kernels + copies / memsets, from
torch's profiler), and for the occupancy forms the decoder's share: the layout, cells and decoder calls get_frame_occ
makes, timed alone on the step's latents, over the step's median.  A report, not a gate."""
import argparse
import os

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')  # before the HIP runtime loads: objectcentricocccompletion_amd/graph.py
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_occ_export import count_launches, fmt, timed   # noqa: E402 (the same measuring functions)
from time_online import tracklets                        # noqa: E402 (the same synthetic tracklets)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--slots', type=int, nargs='+', default=[1, 16, 64])
    ap.add_argument('--frame', type=int, default=50)
    ap.add_argument('--points', type=int, default=256, help='points per frame and tracklet')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the table to this markdown file')
    args = ap.parse_args()
    import torch
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (registers)
    from objectcentricocccompletion_amd.occ import occ_base, occ_ops
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is nothing to time without one'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    cfg = ococcnet_model_cfg()
    cfg['test_cfg']['test_occ_iou'] = False
    rh = DETECTORS.build(cfg).to(dev).eval().roi_head
    ae = rh.bbox_head.occ_ae_head
    dec = ae.occ_decoder
    t = args.frame
    lines = ['| tracklets | path | device events, ms: median (min - max) | host clock, ms | launches: kernels + copies | '
             'cells decoded / returned | decoder share |', '|---|---|---|---|---|---|---|']

    def shape(slots):
        """the forms of one tracklet count: [(name, description, call)], the cells decoded and the rows returned"""
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

        def step(occ, kernel=True):
            state.cache.pos.fill_(t)
            state.cache.pos_host[:] = [t] * slots
            occ_base.OCC_FRAME_KERNEL = kernel
            try:
                return rh.simple_test_step(xyz, feats, batch, boxes, scores, labels, slot, state, **({'occ': True} if occ else {}))
            finally:
                occ_base.OCC_FRAME_KERNEL = True

        first = step(True)
        rois = torch.cat([torch.arange(slots, device=dev, dtype=boxes.dtype)[:, None], boxes[:, :7]], 1)
        latents = first['fused_roi_feats']

        def decode():
            sizes, dims, start, total = occ_ops.dense_grid_layout(rois[:, 4:7], ae.voxel_size, ae.scale_wlh, ae.offset_wlh)
            centers, index = occ_ops.dense_grid_cells(sizes, dims, start, ae.voxel_size, 0, total, total)
            return dec.forward(latents, centers, index), total

        forms = [('plain', '`simple_test_step`', lambda: step(False)),
                 ('kernel', '`simple_test_step(occ=True)`, `csrc/occ_frame.hip`', lambda: step(True)),
                 ('chain', '`simple_test_step(occ=True)`, `OCOCC_OCC_FRAME_KERNEL=0`', lambda: step(True, False)),
                 ('decode', 'layout, cells and decoder of `get_frame_occ` alone', decode)]
        return forms, decode()[1], first['occ'].size(0)

    with torch.no_grad():
        shapes = []
        for slots in args.slots:                      # the end-to-end figures first, the profiler off
            forms, cells, rows = shape(slots)
            for _ in range(args.warmup):
                for _, _, fn in forms:
                    fn()
            times = {name: ([], []) for name, _, _ in forms}
            for _ in range(args.reps):                # alternating: drift of the shared host hits all alike
                for name, _, fn in forms:
                    e, h = timed(fn, 1)
                    times[name][0].extend(e)
                    times[name][1].extend(h)
            shapes.append((slots, forms, cells, rows, times))
        for slots, forms, cells, rows, times in shapes:   # then the launches of one call each, under the profiler
            dec_med = statistics.median(times['decode'][0])
            for name, what, fn in forms:
                kernels, copies = count_launches(fn)
                e, h = times[name]
                share = f'{100 * dec_med / statistics.median(e):.0f} %' if name in ('kernel', 'chain') else ''
                shown = f'{cells} / {rows}' if name in ('kernel', 'chain') else (f'{cells} / -' if name == 'decode' else '')
                lines.append(f'| {slots} | {what} | {fmt(e)} | {fmt(h)} | {kernels} + {copies} | {shown} | {share} |')
                print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
