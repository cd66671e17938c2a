"""Time the sample masks of OccBBoxHead.loss_occ's train_cfg variants on the device:

  masks   occ_ops.occ_loss_masks (csrc/occ_loss_masks.hip, one launch) against occ_ops.occ_loss_masks_aten (the operator
          chain), all three flags on, at the test scene's 44 RoIs x 64 samples and at 64 tracklets x 32 frames x 512
          samples; the two forms alternate in one process, device events around `--inner` calls, 7 repeats each,
          median (min - max) per call
  step    the training step of `bench.py --workload ococcnet` (same model, batch, optimiser and host timing) with no
          switch on and with all four (fused_mode='concat_residual'), `--steps` steps after `--warmup`

Prints one JSON line per measurement.  usage: python tools/time_loss_variants.py [--skip-step] [--tracklets 4]"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')  # see objectcentricocccompletion_amd/graph.py

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def mask_inputs(M, K, dev):
    g = torch.Generator().manual_seed(M * 1000 + K)
    size = torch.rand(M, 3, generator=g) * 2 + 1.5
    xyz = (torch.rand(M, K, 3, generator=g) - 0.5) * size[:, None, :] * 1.3
    return dict(score=torch.rand(M, generator=g).to(dev), labels=torch.randint(0, 2, (M * K,), generator=g).to(dev),
                xyz=xyz.view(-1, 3).to(dev), box_size=size.to(dev), ori_logits=torch.randn(M * K, generator=g).to(dev))


def time_masks(dev, inner, repeats=7):
    from objectcentricocccompletion_amd.occ import occ_ops
    forms = (('kernel', occ_ops.occ_loss_masks), ('chain', occ_ops.occ_loss_masks_aten))
    for what, (M, K) in (('test scene', (44, 64)), ('64 tracklets x 32 frames', (64 * 32, 512))):
        case = mask_inputs(M, K, dev)
        call = lambda fn: fn(case['score'], 0.4, case['labels'], xyz=case['xyz'], box_size=case['box_size'],
                             ori_logits=case['ori_logits'], pos_thresh=0.5, outside=True, observed=True, unmatched=True)
        for _, fn in forms:   # warm-up
            for _ in range(3):
                call(fn)
        times = {name: [] for name, _ in forms}
        for _ in range(repeats):
            for name, fn in forms:   # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(inner):
                    call(fn)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / inner)
        for name, t in times.items():
            print(json.dumps({'measurement': 'masks', 'shape': what, 'rows': M * K, 'form': name, 'repeats': repeats,
                              'inner': inner, 'ms_median': round(statistics.median(t), 5), 'ms_min': round(min(t), 5),
                              'ms_max': round(max(t), 5)}), flush=True)


def time_step(dev, tracklets, steps, warmup):
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401
    from objectcentricocccompletion_amd.occ.occ_base import OccDecoder
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.optim import AdamW
    from objectcentricocccompletion_amd.registry import DETECTORS
    from objectcentricocccompletion_amd.synthetic import synthetic_training_batch
    switches = ('contrastive_loss', 'residual_loss', 'no_loss_for_outside', 'no_loss_for_observed_feats')
    for name, on in (('no switch', False), ('all four', True)):
        torch.manual_seed(0)
        cfg = ococcnet_model_cfg()
        cfg['train_cfg']['random_shift_frame_inds'] = False
        for k in switches:
            cfg['train_cfg'][k] = on
        if on:
            cfg['roi_head']['bbox_head']['fused_mode'] = 'concat_residual'
        model = DETECTORS.build(cfg).to(dev).train()
        for m in model.modules():
            if isinstance(m, OccDecoder):
                m.compute_dtype = torch.bfloat16
        assert all(model.roi_head.bbox_head.train_cfg.get(k, False) == on for k in switches)
        params = [p for p in model.parameters() if p.requires_grad]
        opt = AdamW(params, lr=1e-6)
        batch = synthetic_training_batch(tracklets, 32, pts_per_frame=64, occ_queries=512, seed=0, device=dev)
        keys = []

        def step():
            opt.zero_grad(set_to_none=True)
            losses = model(return_loss=True, **batch)
            keys[:] = sorted(losses)
            total = sum(v.mean() for k, v in losses.items() if 'loss' in k)   # tools/train.py
            total.backward()
            opt.step()

        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({'measurement': 'step', 'switches': name, 'tracklets': tracklets, 'steps': steps, 'warmup': warmup,
                          'ms_per_step': round(dt / steps * 1e3, 3), 'new_keys': [k for k in keys if k in (
                              'loss_contrastive_feats', 'loss_rcnn_occ_residual', 'num_unmatched')]}), flush=True)
        del model, opt, params, batch
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--tracklets', type=int, default=4)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--skip-step', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    time_masks(dev, args.inner)
    if not args.skip_step:
        time_step(dev, args.tracklets, args.steps, args.warmup)


if __name__ == '__main__':
    main()
