#!/usr/bin/env python3
"""Online inference replayed from RAW data: the tracker's result (.bin) and the scene clouds of a track-input yaml
(tools/ctrl/data_configs/*.yaml: bin_path, mm_data_root with idx2timestamp.pkl / idx2contextname.pkl and the velodyne
clouds) stepped through frame by frame, the way the method is deployed -- no track-input database, no per-tracklet files:

    python tools/online_raw.py <config> <checkpoint> <raw.yaml> [--slots 64] [--out FILE.bin] [--poses poses.pkl] [--chunk T]
                               [--save-occ DIR] [--step-tuning N [--step-tuning-samples S]] [--cfg-options k=v ...]
                               [--save-merged DIR [--merged-use-dim 5] [--merged-score-threshold 0] [--merged-drop-observed]
                                [--merged-per-call]]

Per segment and frame, in time order: the frame's scene cloud is loaded once, every track that starts at the frame gets a
free slot of the temporal K/V cache, TrackletRoIHeadOCC.simple_test_scene_step refines all live tracks in one call (crop,
pose transform, decoration, range filter and cap on the device: csrc/scene_rows.hip), and a track's slot is released after
its last frame.  With --chunk T, T consecutive timestamps go into one TrackletRoIHeadOCC.simple_test_scene_steps call (the
rows of T clouds from one count, one read-back and one fill launch, one head pass), slots given before and released after
the call.  More live tracks than slots is an error that names --slots.  The cache is chosen from the longest track as
simple_test_online chooses it: plain up to 256 frames, a ring with test_cfg.attn_window_size, else a long cache.

The refined objects (``boxes_ego``: each in its own frame's ego frame) are written as a Waymo metrics file; an object whose
enlarged box held no point keeps the tracker's box and score, as do objects of types the yaml's ``type`` list leaves out.
With --save-occ DIR every step also returns the completed occupancy of its frame (simple_test_scene_step(..., occ=True):
``occ_ego``, csrc/occ_frame.hip) and the tool writes ``<DIR>/<segment>/<timestamp>/<type>_<id>.bin`` per frame and object,
float32 [n, 4]: the cells in the frame's ego frame and the object's refined score of that frame in column 3 -- the layout
tools/test.py --save-occ writes and occ_export.load_frame_occ reads.  Boxes, scores and cells of a frame come down in one copy.
With --save-merged DIR every step also returns the occupancy-enhanced cloud of its frame (simple_test_scene_step(...,
merged=...): ``points_merged``, csrc/occ_merge.hip) and the tool writes ``<DIR>/<segment>/<timestamp>.bin`` per replayed
frame, float32 [N + K, D + 2]: the first D columns of the frame's cloud with two zero columns, then the cells of the
frame's objects whose score passes --merged-score-threshold as x, y, z, D - 3 zeros, score, 1 -- the array
pipelines.LoadPointsAndOccPredFromFile builds from the cloud file and the --save-occ files of the frame.
--chunk T with --save-merged needs --merged-per-call: the T clouds of a call are then merged by ONE
TrackletRoIHeadOCC.simple_test_scene_steps_merged call (occ_ops.occ_merge_frames: one count launch, one read-back, one
fill launch for the T clouds) and cut into the same per-timestamp files at ``merged_offsets``.
Config and checkpoint are loaded as tools/test.py loads them."""
import argparse
import os

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')  # before the HIP runtime loads: objectcentricocccompletion_amd/graph.py
import pickle
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WAYMO_TYPE_TO_LABEL = {1: 0, 2: 1, 4: 2}     # vehicle, pedestrian, cyclist -> index into ('Car', 'Pedestrian', 'Cyclist')


def choose_cache(roi_head, longest):
    """the cache keywords of online_begin for tracks of up to ``longest`` frames, as simple_test_online picks them"""
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ.layers import TemporalCache
    window = roi_head.test_cfg.get('attn_window_size', -1)
    if longest <= 256:
        return dict(cap=max(longest, 1))
    if window > 0:
        return dict(cap=window, ring=True)
    if longest <= TemporalCache.MAX_LONG_CAP:
        return dict(cap=longest, long=True)
    raise L.OcoccError(f'a track of {longest} frames without test_cfg.attn_window_size: the K/V cache of online inference '
                       f'holds at most {TemporalCache.MAX_LONG_CAP} frames of history')


def replay(model, raw_yaml, slots=64, out=None, poses=None, device=None, save_occ=None, save_merged=None, merged=True,
           chunk=1, merged_per_call=False):
    """``model``: a TrackletDetectorOCC in eval mode on a ROCm device; ``raw_yaml``: the track-input yaml (path or mapping,
    ctrl_prep.load_config); ``poses``: {timestamp: 4x4 ego -> world} or the path of its pickle (default: the yaml's
    ``poses_path``, else <mm_data_root>/poses.pkl).  Returns (records, state): one record per object of the tracker's
    file, tracks in order of first appearance and frames ascending -- dict(segment, id, type, timestamp, box [7] f32 in the
    frame's ego frame, score, num_points: the points in the enlarged box before the cap, refined: whether the head's
    result was taken) -- and the OnlineState, every slot released.  With ``out`` the records are written there as a Waymo
    metrics file.  With ``save_occ`` (a directory) the completed occupancy of every refined frame is written below it, one
    file per frame and object (occ_export.write_tracklet_occ), and every record gets ``occ_cells``, the rows of its file.
    With ``save_merged`` (a directory) the occupancy-enhanced cloud of every replayed frame is written to
    <save_merged>/<segment>/<timestamp>.bin (``merged``: True or the dict simple_test_scene_step takes), and every record
    gets ``merged_cells``, the cells of its object in that file.
    ``chunk`` = T > 1: T consecutive timestamps of a segment per simple_test_scene_steps call, rows slot-major (the last call
    of a segment takes the rest); a track that starts inside the T timestamps has its slot before the call, one that ends
    inside them gives it back after the call, so the call needs a slot for every track live anywhere in it.  Records and
    files are those of chunk = 1.  ``chunk`` > 1 with ``save_merged`` is refused unless ``merged_per_call`` is set: the call
    is then simple_test_scene_steps_merged, which merges the T clouds of the call at once, and the files of its timestamps
    are cut from ``points_merged`` at ``merged_offsets`` -- still one read-back per call."""
    import numpy as np
    import torch
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd import ctrl_prep, occ_export, waymo_io
    chunk = int(chunk)
    if chunk < 1 or (chunk > 1 and save_merged and not merged_per_call):
        raise ValueError('chunk is the number of timestamps per call, an int >= 1, and 1 with save_merged unless '
                         'merged_per_call (--merged-per-call) is set')
    if merged_per_call and not save_merged:
        raise ValueError('merged_per_call goes with save_merged')
    cfg, _ = ctrl_prep.load_config(raw_yaml)
    rh = model.roi_head
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    tracklets = waymo_io.generate_tracklets(waymo_io.read_bin(ctrl_prep.bin_path_for_split(cfg)))
    refine_types = set(cfg.get('type') or (1, 2, 4))
    mm_root = cfg.get('mm_data_root', ctrl_prep.MM_DATA_ROOT)
    ts2idx, _ = ctrl_prep.load_frame_index(mm_root)
    pc_root = ctrl_prep.velodyne_dir(cfg)
    if poses is None or isinstance(poses, (str, os.PathLike)):
        with open(poses or cfg.get('poses_path') or os.path.join(mm_root, 'poses.pkl'), 'rb') as f:
            poses = pickle.load(f)
    live = [k for k, t in enumerate(tracklets) if t.type in refine_types and len(t)]
    state = rh.online_begin(int(slots), dev, **choose_cache(rh, max((len(tracklets[k]) for k in live), default=1)))
    boxes_out = [t.boxes[:, :7].clone() for t in tracklets]
    scores_out = [t.scores.clone().float() for t in tracklets]
    num_points = [[0] * len(t) for t in tracklets]
    refined = [[False] * len(t) for t in tracklets]
    occ_cells = [[0] * len(t) for t in tracklets]
    merged_cells = [[0] * len(t) for t in tracklets]
    step_kw = dict(**({'occ': True} if save_occ else {}), **({'merged': merged} if save_merged else {}))
    by_seg = defaultdict(list)
    for k in live:
        by_seg[tracklets[k].segment_name].append(k)
    for seg, ks in by_seg.items():
        at = defaultdict(list)                       # timestamp -> [(tracklet, position in the tracklet)]
        for k in ks:
            for i, ts in enumerate(tracklets[k].ts_list):
                at[ts].append((k, i))
        missing = [ts for ts in at if ts not in ts2idx or ts not in poses]
        if missing:
            raise KeyError(f'{len(missing)} timestamps of segment {seg} have no frame in idx2timestamp.pkl or no pose '
                           f'(e.g. {sorted(missing)[0]})')
        free, slot_of = list(range(state.slots))[::-1], {}
        stamps = sorted(at)
        for c0 in range(0, len(stamps), chunk):      # `chunk` timestamps per call, the last call takes the rest
            group = stamps[c0:c0 + chunk]
            runs = {}                                # tracklet -> [(cloud of the call, position in the tracklet)], in time order
            for f, ts in enumerate(group):
                for k, i in at[ts]:
                    if i == 0:
                        if not free:
                            raise L.OcoccError(f'segment {seg} has more than {state.slots} live tracks at timestamp {ts}: '
                                               'raise --slots')
                        slot_of[k] = free.pop()
                    runs.setdefault(k, []).append((f, i))
            rows = [(k, i, f) for k, run in runs.items() for f, i in run]      # slot-major (one frame: the frame's order)
            clouds = [np.fromfile(os.path.join(pc_root, f'{ts2idx[ts]}.bin'), dtype=np.float32).reshape(-1, 6) for ts in group]
            boxes = torch.stack([tracklets[k].boxes[i, :7].float() for k, i, _ in rows]).to(dev)
            scores = torch.stack([tracklets[k].scores[i].float() for k, i, _ in rows]).to(dev)
            labels = torch.tensor([WAYMO_TYPE_TO_LABEL[tracklets[k].type] for k, _, _ in rows], dtype=torch.long).to(dev)
            if chunk == 1:
                res = rh.simple_test_scene_step(torch.from_numpy(clouds[0]).to(dev), np.asarray(poses[group[0]], dtype=np.float64),
                                                boxes, scores, labels, [slot_of[k] for k, _, _ in rows], state, **step_kw)
            else:                                    # the clouds of the call: one host -> device copy
                steps = rh.simple_test_scene_steps_merged if save_merged else rh.simple_test_scene_steps
                res = steps(torch.from_numpy(np.concatenate(clouds)).to(dev), [len(c) for c in clouds],
                            np.stack([np.asarray(poses[ts], dtype=np.float64) for ts in group]), boxes, scores, labels,
                            [f for _, _, f in rows], [slot_of[k] for k, _, _ in rows], state,
                            **({'merged': merged} if save_merged else step_kw))
            valid = res['valid'].to(dev).bool()
            back = torch.cat([res['boxes_ego'], torch.where(valid, res['scores'].float(), scores)[:, None],
                              valid[:, None].float()], 1)
            if save_occ or save_merged:                                   # boxes, scores, cells, cloud: still one read-back per call
                parts = [back] + ([res['occ_ego']] if save_occ else []) + ([res['points_merged']] if save_merged else [])
                flat = torch.cat([p.reshape(-1) for p in parts]).cpu().split([p.numel() for p in parts])
                back = flat[0].view(-1, 9)
                if save_occ:
                    cells = flat[1].view(-1, 4).numpy()
                    cuts = np.cumsum([0] + list(res['occ_counts']))
                if save_merged:                                           # a file per timestamp of the call
                    cloud = flat[-1].numpy()
                    width = res['points_merged'].size(1)
                    at_row = res.get('merged_offsets', [0, res['points_merged'].size(0)])
                    for f, ts in enumerate(group):
                        path = os.path.join(save_merged, str(seg), f'{ts}.bin')
                        os.makedirs(os.path.dirname(path), exist_ok=True)
                        cloud[at_row[f] * width:at_row[f + 1] * width].tofile(path)
            else:
                back = back.cpu()                                         # one read-back per call
            done = []
            for r, (k, i, f) in enumerate(rows):
                boxes_out[k][i], scores_out[k][i] = back[r, :7], back[r, 7]
                refined[k][i], num_points[k][i] = bool(back[r, 8]), int(res['num_points'][r])
                if save_occ:
                    mine = cells[cuts[r]:cuts[r + 1]].copy()
                    mine[:, 3] = float(back[r, 7])                        # the score column of the exported files
                    occ_export.write_tracklet_occ(save_occ, seg, [group[f]], tracklets[k].type, tracklets[k].id, mine,
                                                  [len(mine)])
                    occ_cells[k][i] = len(mine)
                if save_merged:
                    merged_cells[k][i] = int(res['merged_counts'][r])
                if i == len(tracklets[k]) - 1:
                    done.append(slot_of.pop(k))
            if done:
                state.reset(done)
                free.extend(done)
    records, chunks = [], []
    for k, t in enumerate(tracklets):
        b, s = boxes_out[k].numpy(), scores_out[k].numpy()
        for i, ts in enumerate(t.ts_list):
            records.append(dict(segment=t.segment_name, id=t.id, type=t.type, timestamp=ts, box=b[i], score=float(s[i]),
                                num_points=num_points[k][i], refined=refined[k][i]))
            if save_occ:
                records[-1]['occ_cells'] = occ_cells[k][i]
            if save_merged:
                records[-1]['merged_cells'] = merged_cells[k][i]
            if out:
                chunks.append(waymo_io._f_bytes(1, waymo_io.lidar2waymo_box(b[i], s[i], t.type, t.segment_name, ts, t.id)))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'wb') as f:
            f.write(b''.join(chunks))
    return records, state


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('config', help='model config file path (tools/test.py)')
    ap.add_argument('checkpoint', help='checkpoint file (tools/train.py: a dict with state_dict)')
    ap.add_argument('raw_yaml', help='track-input yaml: bin_path, mm_data_root, split, type')
    ap.add_argument('--slots', type=int, default=64, help='tracks followed at the same time (9.4 MB of K/V cache each at 256 frames)')
    ap.add_argument('--out', default=None, help='the refined objects as a Waymo metrics file (default: <bin stem>_online.bin)')
    ap.add_argument('--poses', default=None, help='poses.pkl: {timestamp: 4x4 ego -> world} (default: the yaml\'s poses_path, '
                    'else <mm_data_root>/poses.pkl)')
    ap.add_argument('--save-occ', metavar='DIR', default=None,
                    help='write the completed occupancy of every frame and object below DIR: <segment>/<timestamp>/<type>_<id>.bin, '
                    'float32 [n, 4] in the frame\'s ego frame, the refined score in column 3 (occ_export.load_frame_occ reads it)')
    ap.add_argument('--save-merged', metavar='DIR', default=None,
                    help='write the occupancy-enhanced cloud of every replayed frame to DIR/<segment>/<timestamp>.bin, float32 '
                    '[N + K, D + 2]: the cloud\'s first D columns, 0, 0, then the surviving cells as x, y, z, zeros, score, 1')
    ap.add_argument('--merged-use-dim', type=int, metavar='D', default=None,
                    help='columns of the cloud kept under --save-merged (default 5, or test_cfg.online_merged)')
    ap.add_argument('--merged-score-threshold', type=float, metavar='T', default=None,
                    help='a cell is kept iff its object\'s score of the frame is > T (default 0, or test_cfg.online_merged)')
    ap.add_argument('--merged-drop-observed', action='store_true',
                    help='leave out the cells a real point of the frame fell into')
    ap.add_argument('--chunk', type=int, metavar='T', default=1,
                    help='T consecutive timestamps of a segment per call (simple_test_scene_steps: the rows of T clouds from one '
                    'count launch, one read-back and one fill launch, one head pass); with --save-merged only together '
                    'with --merged-per-call')
    ap.add_argument('--merged-per-call', action='store_true',
                    help='with --chunk T and --save-merged: merge the T clouds of a call at once '
                    '(simple_test_scene_steps_merged) and cut the per-timestamp files from the result')
    ap.add_argument('--step-tuning', type=int, metavar='N', default=None,
                    help='tune the fused shape latent of every live track against the frame\'s own points with N Adam steps '
                    'inside the step (sets test_cfg.online_step_tuning = dict(num_iter=N, downsample_size=S, '
                    'balance_sample=True, seed=0); boxes, scores and --save-occ files then come from the tuned latent)')
    ap.add_argument('--step-tuning-samples', type=int, metavar='S', default=None,
                    help='at most S sampled cells per RoI under --step-tuning (default -1: no limit)')
    ap.add_argument('--cfg-options', nargs='+', default=[], help='k=v overrides merged into the config')
    args = ap.parse_args(argv)
    if args.slots < 1:
        ap.error('--slots takes a number of tracks >= 1')
    if args.chunk < 1:
        ap.error('--chunk takes a number of timestamps >= 1')
    if args.merged_per_call and args.save_merged is None:
        ap.error('--merged-per-call goes with --save-merged')
    if args.chunk > 1 and args.save_merged is not None and not args.merged_per_call:
        ap.error('--chunk above 1 goes with --save-merged only under --merged-per-call: the occupancy-enhanced clouds of '
                 'a call are then merged at once')
    if args.step_tuning is not None and args.step_tuning < 0:
        ap.error('--step-tuning takes a number of iterations >= 0')
    if args.step_tuning_samples is not None and args.step_tuning is None:
        ap.error('--step-tuning-samples goes with --step-tuning')
    if args.save_merged is None and (args.merged_use_dim is not None or args.merged_score_threshold is not None
                                     or args.merged_drop_observed):
        ap.error('--merged-use-dim, --merged-score-threshold and --merged-drop-observed go with --save-merged')
    if args.merged_use_dim is not None and not 3 <= args.merged_use_dim <= 6:
        ap.error('--merged-use-dim takes 3 to 6 columns of the six a cloud file holds')
    return args


def merged_arg(args):
    """the ``merged`` argument of simple_test_scene_step from the --merged-* options: only what was given overrides
    test_cfg.online_merged"""
    cfg = {}
    if args.merged_use_dim is not None:
        cfg['use_dim'] = args.merged_use_dim
    if args.merged_score_threshold is not None:
        cfg['score_threshold'] = args.merged_score_threshold
    if args.merged_drop_observed:
        cfg['drop_observed'] = True
    return cfg or True


def main(argv=None):
    args = parse_args(argv)
    import importlib.util

    import torch
    from objectcentricocccompletion_amd import config, ctrl_prep, heads, point_pool, roi_head  # noqa: F401 (registers)
    from objectcentricocccompletion_amd.registry import DETECTORS
    spec = importlib.util.spec_from_file_location('ococc_tools_test', os.path.join(ROOT, 'tools', 'test.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    cfg = config.fromfile(args.config)
    config.merge_from_dict(cfg, tool.parse_kv(args.cfg_options))
    if args.step_tuning is not None:
        config.merge_from_dict(cfg, {'model.test_cfg.online_step_tuning': dict(
            num_iter=args.step_tuning, downsample_size=-1 if args.step_tuning_samples is None else args.step_tuning_samples,
            balance_sample=True, seed=0)})
    dev = torch.device('cuda', torch.cuda.current_device())
    model = DETECTORS.build(cfg['model']).to(dev)
    ck = torch.load(args.checkpoint, map_location=dev)
    model.load_state_dict(ck['state_dict'] if 'state_dict' in ck else ck)
    model.eval()
    raw, _ = ctrl_prep.load_config(args.raw_yaml)
    out = args.out or os.path.splitext(ctrl_prep.bin_path_for_split(raw))[0] + '_online.bin'
    records, _ = replay(model, args.raw_yaml, slots=args.slots, out=out, poses=args.poses, device=dev, save_occ=args.save_occ,
                        save_merged=args.save_merged, merged=merged_arg(args), chunk=args.chunk,
                        merged_per_call=args.merged_per_call)
    print(f'{len(records)} objects, {sum(r["refined"] for r in records)} refined; wrote {out}')
    if args.save_occ:
        print(f'{sum(r.get("occ_cells", 0) for r in records)} occupancy cells in {args.save_occ}')
    if args.save_merged:
        print(f'{sum(r.get("merged_cells", 0) for r in records)} occupancy cells merged into the clouds in {args.save_merged}')
    return out


if __name__ == '__main__':
    main()
