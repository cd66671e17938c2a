#!/usr/bin/env python3
"""Dense decode for the occupancy export, timed on the MI355X: OccAutoEncoder.get_occ (the ATen chain around the decoder)
against get_occ_packed (csrc/occ_export.hip) on the same weights and RoIs, 8 and 200 RoIs of vehicle size.
    python tools/time_occ_export.py [--rois 8 200] [--reps 9] [--out profiles/occ_export.md]
Per size: both paths are warmed up, checked to give the same bytes, then timed alternately; a call is timed with device
events around it and with the host clock (both calls end in a read-back, i.e. are synchronous); the median, minimum and
maximum of the repetitions are reported.  Kernel launches per call come from a torch.profiler run of its own, host
synchronisations from torch's sync-debug warnings.  `decoder alone` is the time of the decoder's forward() on the cells
of the same RoIs, already laid out: what either path cannot go below."""
import argparse
import os

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')  # before the HIP runtime loads: objectcentricocccompletion_amd/graph.py
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def vehicle_rois(n, dev, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    size = torch.tensor([2.0, 4.6, 1.7]) + (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([0.4, 1.0, 0.4])
    return torch.cat([torch.zeros(n, 1), torch.rand(n, 3, generator=g) * 100 - 50, size,
                      torch.rand(n, 1, generator=g) * 6.28 - 3.14], 1).to(dev)


def timed(fn, reps):
    import torch
    ev, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return ev, host


def count_syncs(fn):
    import torch
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode('default')
    return sum('synchroniz' in str(x.message) for x in w)


def count_launches(fn):
    """(kernels, memcpy / memset) on the device during one call, from torch.profiler's device events; a profiler that
    records no device activity is an error: the launch count is one of the figures this tool is for"""
    import torch
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    dev_events = [e for e in prof.events() if e.device_type == DeviceType.CUDA]
    if not dev_events:
        raise RuntimeError('torch.profiler recorded no device activity: the launches cannot be counted here')
    copies = [e for e in dev_events if e.name.lower().startswith(('memcpy', 'memset'))]
    return len(dev_events) - len(copies), len(copies)


def fmt(v):
    return f'{statistics.median(v):.3f} ({min(v):.3f} - {max(v):.3f})'


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rois', type=int, nargs='+', default=[8, 200])
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the tables to this markdown file')
    args = ap.parse_args()
    import torch
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (registers)
    from objectcentricocccompletion_amd.occ import occ_ops
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is nothing to time without one'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    ae = DETECTORS.build(ococcnet_model_cfg()).to(dev).eval().roi_head.bbox_head.occ_ae_head
    dec = ae.occ_decoder
    lines = ['| RoIs | cells | occupied | path | device events, ms: median (min - max) | host clock, ms | kernel launches '
             '| copies / memsets | host synchronisations |', '|---|---|---|---|---|---|---|---|---|']
    for n in args.rois:
        rois = vehicle_rois(n, dev)
        feats = torch.randn(n, dec.roi_feature_channels, generator=torch.Generator().manual_seed(1)).to(dev)
        old = lambda: ae.get_occ(feats, rois, transform=True)
        new = lambda: ae.get_occ_packed(feats, rois, transform=True)
        sizes, dims, start, total = occ_ops.dense_grid_layout(rois[:, 4:7], ae.voxel_size, ae.scale_wlh, ae.offset_wlh)
        cells = [occ_ops.dense_grid_cells(sizes, dims, start, ae.voxel_size, lo, min(lo + (1 << 20), total), total)
                 for lo in range(0, total, 1 << 20)]

        def mlp():
            with torch.no_grad():
                for c, i in cells:
                    dec(feats, c, i)

        for _ in range(args.warmup):
            a, (b, counts) = old(), new()
            mlp()
        flat = torch.cat([t for s in a for t in s])
        assert torch.equal(flat, b) and counts == [int(t.size(0)) for s in a for t in s], 'the two paths differ'
        t = {'get_occ': ([], []), 'get_occ_packed': ([], []), 'decoder alone': ([], [])}
        for _ in range(args.reps):                       # alternating: drift of the shared host hits all alike
            for name, fn in (('get_occ', old), ('get_occ_packed', new), ('decoder alone', mlp)):
                e, h = timed(fn, 1)
                t[name][0].extend(e)
                t[name][1].extend(h)
        for name, fn in (('get_occ', old), ('get_occ_packed', new), ('decoder alone', mlp)):
            print(f'# {n} RoIs {name}: events {fmt(t[name][0])} ms, host {fmt(t[name][1])} ms', flush=True)
            syncs = count_syncs(fn)
            k, c = count_launches(fn)
            lines.append(f'| {n} | {total} | {int(b.size(0))} | `{name}` | {fmt(t[name][0])} | {fmt(t[name][1])} | {k} | {c} '
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
