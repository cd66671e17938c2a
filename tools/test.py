#!/usr/bin/env python3
"""Test / evaluation entry point with the CLI of the reference's tools/test.py (:23-87):
    python tools/test.py <config> <checkpoint> [--out FILE.pkl] [--save-occ DIR] [--save-gt-occ DIR] [--online [--online-chunk T]] [--eval iou waymo waymo_native] [--matcher {score_first,hungarian}] [--format-only]
                         [--online-tuning N [--tuning-samples S]] [--step-tuning N [--step-tuning-samples S]]
                         [--decoder-dtype {f32,bf16}]
                         [--eval-options k=v ...] [--cfg-options k=v ...] [--launcher {none,pytorch}]
                         [--tmpdir DIR] [--gpu-collect] [--local_rank N]
The test dataset is the config's data.test (the reference's data/waymo layout); with --data-root DIR it reads the tree
tools/make_synthetic_dataset.py writes (file names as in tools/train.py).  The checkpoint is ``ck['state_dict']`` as
tools/train.py writes it (the reference's parameter names).  The model runs in eval mode under torch.no_grad(), one
tracklet at a time (batch 1, as the reference asserts); test_cfg.tta works as in model(return_loss=False).  Every
tracklet's pipeline draws its random numbers (point subsets, point shuffle) from a seed of its own (--seed + index), so a
shard computes what one process computes for the same tracklets.

Several GPUs (--launcher pytorch, one process per GPU, tools/dist_test.sh): rank r evaluates the contiguous shard
dist.shard_range(len(dataset), r, world) -- the reference's multi_gpu_test_sequential, a tracklet's results stay
together -- and dist.collect_results joins the results on rank 0 in dataset order (pickles in --tmpdir by default,
an all-gather of pickled byte tensors with --gpu-collect).  Only rank 0 writes --out and evaluates.
Reference flags this package has no use for (--show, --show-dir, --fuse-conv-bn, --deterministic) are accepted and
ignored with a warning."""
import argparse
import ast
import os

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')  # before the HIP runtime loads: objectcentricocccompletion_amd/graph.py
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRICS = ('iou', 'waymo', 'waymo_native')


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Test (and evaluate) an OcOccNet checkpoint (MI355X)')
    ap.add_argument('config', help='test config file path')
    ap.add_argument('checkpoint', help='checkpoint file (tools/train.py: a dict with state_dict)')
    ap.add_argument('--out', help='output result file in pickle format: one result per tracklet, in dataset order')
    ap.add_argument('--fuse-conv-bn', action='store_true', help='ignored: the model has no conv + BN pair')
    ap.add_argument('--format-only', action='store_true', help='write the Waymo result file without evaluating it')
    ap.add_argument('--eval', type=str, nargs='+', choices=METRICS, help='metrics: iou (occupancy), waymo (detection, needs the Waymo tool), waymo_native (detection, '
                    'HIP matching kernels: objectcentricocccompletion_amd/waymo_metrics.py)')
    ap.add_argument('--matcher', choices=('score_first', 'hungarian'), default=None,
                    help='matcher of --eval waymo_native (default score_first; hungarian: maximum total overlap per score cutoff)')
    ap.add_argument('--show', action='store_true', help='ignored: no visualisation here')
    ap.add_argument('--show-dir', help='ignored: no visualisation here')
    ap.add_argument('--gpu-collect', action='store_true', help='collect the ranks\' results by an all-gather')
    ap.add_argument('--tmpdir', help='directory of the ranks\' result pickles (default: a fresh temporary one)')
    ap.add_argument('--seed', type=int, default=0, help='base seed of the per-tracklet pipeline draws')
    ap.add_argument('--deterministic', action='store_true', help='ignored: there is no cuDNN here')
    ap.add_argument('--cfg-options', nargs='+', default=[], help='k=v overrides merged into the config')
    ap.add_argument('--options', nargs='+', help='deprecated spelling of --eval-options')
    ap.add_argument('--eval-options', nargs='+', help='k=v keyword arguments of dataset.evaluate()')
    ap.add_argument('--launcher', choices=['none', 'pytorch'], default='none')
    ap.add_argument('--local_rank', '--local-rank', type=int, default=0)
    ap.add_argument('--dist-backend', choices=['nccl', 'gloo'], default=None,
                    help='process-group backend (default: nccl, i.e. RCCL, with a GPU)')
    ap.add_argument('--data-root', default=None, help='tree with tracklet_data/*.pkl, poses.pkl, occ_gt/ (tools/train.py)')
    ap.add_argument('--proposals', default='tracklet_data/synth_training.pkl')
    ap.add_argument('--candidates', default='tracklet_data/synth_training_gt_candidates.pkl')
    ap.add_argument('--occ-root', default='occ_gt')
    ap.add_argument('--save-occ', metavar='DIR', default=None,
                    help='export the completed occupancy: DIR/<segment>/<timestamp>/<type>_<id>.bin per object and frame, '
                    'float32 [n, 4] (sets test_cfg.occ_save_root and test_cfg.save_occ; read back with '
                    'objectcentricocccompletion_amd.occ_export.load_frame_occ)')
    ap.add_argument('--save-gt-occ', metavar='DIR', default=None,
                    help='export the annotated occupancy of the matched ground-truth tracks, cropped to the proposal boxes: '
                    'the same layout and format under DIR, score 1, frames with a GT box only (sets '
                    'test_cfg.gt_occ_save_root and test_cfg.save_gt_occ)')
    ap.add_argument('--online', action='store_true',
                    help='refine every tracklet frame by frame over a temporal K/V cache, the way the method is deployed '
                    '(sets test_cfg.online; the tracklet is moved into the ego frame of its FIRST frame, the one an online '
                    'caller knows); metrics and files as without it')
    ap.add_argument('--online-chunk', type=int, metavar='T', default=None,
                    help='with --online: feed T frames of the tracklet per call instead of one (sets test_cfg.online_chunk; '
                    'the same result, one attention launch per layer for the T frames)')
    ap.add_argument('--online-tuning', type=int, metavar='N', default=None,
                    help='tune the fused shape latent of every RoI against its own observation with N Adam steps before the '
                    'heads read it (sets test_cfg.online_tuning = dict(num_iter=N, downsample_size=S, balance_sample=True))')
    ap.add_argument('--tuning-samples', type=int, metavar='S', default=None,
                    help='at most S sampled cells per RoI under --online-tuning (default -1: no limit)')
    ap.add_argument('--step-tuning', type=int, metavar='N', default=None,
                    help='with --online: tune the fused shape latent of every frame against the frame\'s own points with N '
                    'Adam steps inside the step, the sample drawn on HIP kernels and the loss a mean per RoI (sets '
                    'test_cfg.online_step_tuning = dict(num_iter=N, downsample_size=S, balance_sample=True, seed=0))')
    ap.add_argument('--step-tuning-samples', type=int, metavar='S', default=None,
                    help='at most S sampled cells per RoI under --step-tuning (default -1: no limit)')
    ap.add_argument('--decoder-dtype', choices=('f32', 'bf16'), default='f32',
                    help='compute dtype of the occupancy decoder (bf16: the fused decoder and tuning kernels)')
    args = ap.parse_args(argv)
    if args.online and args.online_tuning is not None:
        ap.error('--online-tuning is not built for frame-by-frame inference (--online)')
    if args.online and args.decoder_dtype != 'f32':
        ap.error('--decoder-dtype does not go with --online')
    if args.online_chunk is not None and not args.online:
        ap.error('--online-chunk goes with --online')
    if args.online_chunk is not None and args.online_chunk < 1:
        ap.error('--online-chunk takes a number of frames >= 1')
    if args.tuning_samples is not None and args.online_tuning is None:
        ap.error('--tuning-samples goes with --online-tuning')
    if args.online_tuning is not None and args.online_tuning < 0:
        ap.error('--online-tuning takes a number of iterations >= 0')
    if args.step_tuning is not None and not args.online:
        ap.error('--step-tuning goes with --online (offline: --online-tuning)')
    if args.step_tuning is not None and args.step_tuning < 0:
        ap.error('--step-tuning takes a number of iterations >= 0')
    if args.step_tuning_samples is not None and args.step_tuning is None:
        ap.error('--step-tuning-samples goes with --step-tuning')
    if 'LOCAL_RANK' not in os.environ:
        os.environ['LOCAL_RANK'] = str(args.local_rank)
    if args.matcher and 'waymo_native' not in (args.eval or []):
        ap.error('--matcher goes with --eval waymo_native')
    if args.options and args.eval_options:
        ap.error('--options and --eval-options cannot be both specified')
    if args.options:
        warnings.warn('--options is deprecated in favor of --eval-options')
        args.eval_options = args.options
    for flag in ('show', 'show_dir', 'fuse_conv_bn', 'deterministic'):
        if getattr(args, flag):
            warnings.warn(f'--{flag.replace("_", "-")} is accepted for the reference\'s CLI and ignored here')
    return args


def parse_kv(items):
    """k=v strings -> dict; values through ast.literal_eval where they parse (tools/train.py's --cfg-options)."""
    out = {}
    for kv in items or []:
        k, v = kv.split('=', 1)
        try:
            v = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            pass
        out[k] = v
    return out


def build_test_dataset_cfg(cfg, args):
    """data.test of the config; --data-root points its files at a tree in tools/make_synthetic_dataset.py's layout."""
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_test_data
    ds_cfg = dict(cfg.get('data', {}).get('test') or ococcnet_test_data())
    if args.data_root:
        j = lambda p: os.path.join(args.data_root, p)
        ds_cfg.update(data_root=args.data_root, ann_file=j(args.candidates), tracklet_proposals_file=j(args.proposals),
                      occ_anno_root=j(args.occ_root), pose_file=j('poses.pkl'))
    ds_cfg.pop('samples_per_gpu', None)
    if getattr(args, 'online', False):
        # the frames of a tracklet must share ONE coordinate frame known at its first step: the first frame's ego pose
        ds_cfg['pipeline'] = [dict(step, shared_frame='first') if step.get('type') == 'TrackletPoseTransform' else step
                              for step in ds_cfg['pipeline']]
    return ds_cfg


def to_host(obj):
    """Tensors (also inside Tracklets, lists, dicts) moved to host memory: what is pickled and gathered."""
    import copy
    import torch
    if torch.is_tensor(obj):
        return obj.cpu()
    if isinstance(obj, dict):
        return {k: to_host(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(to_host(v) for v in obj)
    if hasattr(obj, '__dict__') and not isinstance(obj, type):
        new = copy.copy(obj)
        new.__dict__.update({k: to_host(v) for k, v in obj.__dict__.items()})
        return new
    return obj


def run_shard(model, dataset, lo, hi, device, seed=0):
    """model(return_loss=False) on tracklets [lo, hi), one at a time; results in host memory."""
    import numpy as np
    import torch
    from objectcentricocccompletion_amd.pipelines import collate_tracklets
    results = []
    with torch.no_grad():
        for i in range(lo, hi):
            np.random.seed(seed + i)
            torch.manual_seed(seed + i)
            batch = collate_tracklets([dataset[i]], device)
            out = model(return_loss=False, **batch)
            assert len(out) == 1, 'one result per tracklet (batch 1)'
            results.append(to_host(out[0]))
    return results


def main(argv=None):
    args = parse_args(argv)
    assert args.out or args.eval or args.format_only or args.show or args.show_dir or args.save_occ or args.save_gt_occ, (
        'Please specify at least one operation (save/eval/format/show the results) with the argument "--out", "--eval", '
        '"--format-only", "--save-occ", "--save-gt-occ", "--show" or "--show-dir"')
    if args.eval and args.format_only:
        raise ValueError('--eval and --format_only cannot be both specified')
    if args.out is not None and not args.out.endswith(('.pkl', '.pickle')):
        raise ValueError('The output file must be a pkl file.')
    import pickle

    import torch
    from objectcentricocccompletion_amd import config, dataset, heads, point_pool, roi_head  # noqa: F401 (registers)
    from objectcentricocccompletion_amd.dist import collect_results, init_dist, shard_range
    from objectcentricocccompletion_amd.registry import DATASETS, DETECTORS
    from objectcentricocccompletion_amd.sir import check_barriers
    cfg = config.fromfile(args.config)
    config.merge_from_dict(cfg, parse_kv(args.cfg_options))
    if args.save_occ:
        # (ranks hold disjoint tracklets, hence disjoint files: nothing to coordinate beyond makedirs(exist_ok=True))
        os.makedirs(args.save_occ, exist_ok=True)
        config.merge_from_dict(cfg, {'model.test_cfg.occ_save_root': args.save_occ, 'model.test_cfg.save_occ': True})
    if args.save_gt_occ:
        os.makedirs(args.save_gt_occ, exist_ok=True)
        config.merge_from_dict(cfg, {'model.test_cfg.gt_occ_save_root': args.save_gt_occ, 'model.test_cfg.save_gt_occ': True})
    if args.online:
        config.merge_from_dict(cfg, {'model.test_cfg.online': True})
    if args.online_chunk is not None:
        config.merge_from_dict(cfg, {'model.test_cfg.online_chunk': args.online_chunk})
    if args.online_tuning is not None:
        config.merge_from_dict(cfg, {'model.test_cfg.online_tuning': dict(
            num_iter=args.online_tuning, downsample_size=-1 if args.tuning_samples is None else args.tuning_samples,
            balance_sample=True)})
    if args.step_tuning is not None:
        config.merge_from_dict(cfg, {'model.test_cfg.online_step_tuning': dict(
            num_iter=args.step_tuning, downsample_size=-1 if args.step_tuning_samples is None else args.step_tuning_samples,
            balance_sample=True, seed=0)})
    rank, world, local_rank = init_dist(args.dist_backend) if args.launcher == 'pytorch' else (0, 1, 0)
    dev = torch.device('cuda', local_rank % max(torch.cuda.device_count(), 1))
    torch.cuda.set_device(dev)
    ds = DATASETS.build(build_test_dataset_cfg(cfg, args))
    torch.manual_seed(args.seed)
    model = DETECTORS.build(cfg['model']).to(dev)
    ck = torch.load(args.checkpoint, map_location=dev)
    model.load_state_dict(ck['state_dict'] if 'state_dict' in ck else ck)
    model.eval()
    if args.decoder_dtype == 'bf16':
        from objectcentricocccompletion_amd.occ.occ_base import OccDecoder
        for m in model.modules():
            if isinstance(m, OccDecoder):
                m.compute_dtype = torch.bfloat16
    lo, hi = shard_range(len(ds), rank, world)
    t0 = time.perf_counter()
    part = run_shard(model, ds, lo, hi, dev, args.seed)
    torch.cuda.synchronize()
    check_barriers()   # nothing is gathered or written from a run whose one-launch SIR layers could not gather their grids
    if rank == 0:
        print(f'{len(ds)} tracklets, {hi - lo} on rank 0 of {world}: {time.perf_counter() - t0:.2f} s', flush=True)
    outputs = collect_results(part, len(ds), args.tmpdir, args.gpu_collect)
    if rank != 0:
        return None
    if args.out:
        print(f'\nwriting results to {args.out}')
        with open(args.out, 'wb') as f:
            pickle.dump(outputs, f)
    kwargs = parse_kv(args.eval_options)
    if args.format_only:
        from objectcentricocccompletion_amd import waymo_io
        path = waymo_io.convert_tracklet_to_waymo([r['out_tracklets'][0] for r in outputs],
                                                  kwargs.get('pklfile_prefix', 'results'), ds.CLASSES)
        print(f'wrote {path}')
    metrics = None
    if args.eval:
        eval_kwargs = {k: v for k, v in (cfg.get('evaluation') or {}).items()
                       if k not in ('interval', 'tmpdir', 'start', 'gpu_collect', 'save_best', 'rule')}
        eval_kwargs.update(kwargs, metric=args.eval)
        if args.matcher:
            eval_kwargs['matcher'] = args.matcher
        metrics = ds.evaluate(outputs, **eval_kwargs)
        print(metrics, flush=True)
    return metrics


if __name__ == '__main__':
    main()
