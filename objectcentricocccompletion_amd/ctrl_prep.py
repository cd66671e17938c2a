"""Tracklet data preparation -- steps 4 and 5 of the reference's "Tracklet Data Preparation"
(tools/ctrl/generate_track_input.py, tools/ctrl/generate_candidates.py): from a detection / tracking result in Waymo
``.bin`` format to the three inputs WaymoTrackletDatasetWithOcc reads,

    <data_root>/<name>_<split>.pkl                       tracklets in dump format (with num_pts_in_boxes)
    <data_root>/<name>_<split>_database/<seg>--<id>.npy  per tracklet: the per-frame [n, 6] points inside its enlarged boxes
    <data_root>/<name>_<split>_gt_candidates.pkl         per tracklet: the GT tracklets with max IoU > affinity_thresh

The two hot paths are HIP kernels (csrc/tracklet_crop.hip, csrc/tracklet_iou.hip): the reference crops with one
points_in_boxes launch, one mask compaction and one device-to-host copy PER BOX of every frame
(generate_track_input.py:84-99) and scores with one upload, launch and ``.item()`` PER PAIR of tracklets
(generate_candidates.py:61-65, lidar_tracklet.py:210-229); here a batch of frames is one count launch, one read-back and
one fill launch, a segment's P x G affinity matrix one launch and one read-back.

Two more tools of the same family run between the tracker and step 4 (and again on the refined result):
tools/ctrl/extend_tracks.py (extend_tracks: every tracklet extended backward in time by a constant-velocity model, all
tracklets of a file in one launch of csrc/track_extend.hip, the plan made on the host) and tools/ctrl/remove_empty.py
(remove_empty: boxes without a lidar point dropped; the non-empty mode of csrc/tracklet_crop.hip, one launch and one
read-back per batch of frames where the reference has them per box)."""
import os
import os.path as osp
import pickle
from collections import defaultdict

import numpy as np
import torch

from . import _lib as L
from . import waymo_io
from .tracklet import Tracklet

MM_DATA_ROOT = './data/waymo/kitti_format'   # the path the reference hard-codes; config key ``mm_data_root`` overrides
MAX_PROCESSES = 16                            # processes that may hold the GPUs open at the same time
CROP_BATCH_BYTES = 256 << 20                  # point bytes uploaded per crop call: bounds the device memory of a segment
_CROP_BLOCK_TILE = 4096                       # points per workgroup of tracklet_crop_kernel (workspace size)
SPLITS = ('training', 'val', 'test')


# ------------------------------------------------------------------------------------------------ device operators
def crop_frames_packed(points, point_offsets, boxes, box_offsets):
    """points [N, C] f32 of F frames back to back, point_offsets: F + 1 ints (host), boxes [B, 7] f32 (already
    enlarged) grouped by frame, box_offsets: F + 1 ints (host) -> (counts [B] int64 on the HOST, out_index [sum counts]
    int64 on the device): the frame-local indices of the points inside box b, ascending, at
    [scan[b], scan[b + 1]) with scan the exclusive scan of counts.  One count launch, one read-back, one fill launch."""
    L.require_device(points, boxes)
    if points.dim() != 2 or points.size(1) < 3 or points.dtype != torch.float32:
        raise L.OcoccError(f'points must be [N, >= 3] float32, got {tuple(points.shape)} {points.dtype}')
    po, bo = [int(v) for v in point_offsets], [int(v) for v in box_offsets]
    frames = len(po) - 1
    if len(bo) != frames + 1 or frames < 0 or po[0] != 0 or bo[0] != 0 or po[-1] != points.size(0) or bo[-1] != boxes.size(0) \
            or any(b < a for a, b in zip(po, po[1:])) or any(b < a for a, b in zip(bo, bo[1:])):
        raise L.OcoccError('crop_frames: offsets must start at 0, not decrease and end at the row counts')
    dev = points.device
    points = points.contiguous()
    boxes = boxes[:, :7].contiguous().float()
    n, b = points.size(0), boxes.size(0)
    counts = torch.zeros((b,), dtype=torch.int64, device=dev)
    if b == 0 or n == 0 or frames == 0:
        return counts.cpu(), torch.zeros((0,), dtype=torch.int64, device=dev)
    max_pts = max(y - x for x, y in zip(po, po[1:]))
    offs = torch.tensor(po + bo, dtype=torch.int64).to(dev)
    p_off, b_off = offs[:frames + 1], offs[frames + 1:]
    ws_bytes = (max_pts + _CROP_BLOCK_TILE - 1) // _CROP_BLOCK_TILE * 4 * b * 4
    ws = L.workspace(ws_bytes, dev)
    L.check(L.lib.ococc_tracklet_crop_count(L.ptr(points), n, points.size(1), L.ptr(p_off), L.ptr(boxes), b, L.ptr(b_off),
                                            frames, max_pts, L.ptr(counts), L.ptr(ws), ws_bytes, L.stream()),
            'tracklet_crop_count')
    counts_host = counts.cpu()                                   # the read-back
    scan = torch.zeros((b + 1,), dtype=torch.int64)
    torch.cumsum(counts_host, 0, out=scan[1:])
    out_index = torch.empty((int(scan[-1]),), dtype=torch.int64, device=dev)
    if out_index.numel():
        scan_dev = scan.to(dev)
        L.check(L.lib.ococc_tracklet_crop_fill(L.ptr(points), n, points.size(1), L.ptr(p_off), L.ptr(boxes), b, L.ptr(b_off),
                                               frames, max_pts, L.ptr(scan_dev), L.ptr(ws), ws_bytes, L.ptr(out_index),
                                               L.stream()), 'tracklet_crop_fill')
    return counts_host, out_index


def crop_frames(points_list, boxes_list):
    """Per frame f: points_list[f] [n_f, C] f32 and boxes_list[f] [b_f, 7] f32 (already enlarged), device tensors ->
    (counts [B] int64 on the host, index_lists: per box, in frame order, the ascending indices into its frame's points
    of the points inside it -- views of one device tensor).  A point may be in several boxes."""
    if len(points_list) != len(boxes_list):
        raise L.OcoccError('crop_frames: one box tensor per point tensor')
    L.require_device(*points_list, *boxes_list)
    if len(points_list) == 0:
        return torch.zeros((0,), dtype=torch.int64), []
    po = np.concatenate([[0], np.cumsum([p.size(0) for p in points_list])]).tolist()
    bo = np.concatenate([[0], np.cumsum([b.size(0) for b in boxes_list])]).tolist()
    counts, out_index = crop_frames_packed(torch.cat(list(points_list), 0), po, torch.cat([b[:, :7] for b in boxes_list], 0), bo)
    return counts, list(out_index.split(counts.tolist()))


def max_iou_packed(pd_boxes, pd_offsets, pd_frames, gt_boxes, gt_offsets, gt_frames):
    """The boxes of P predicted tracklets back to back [sum Lp, 7] f32 with offsets [P + 1] i32 and frame indices
    [sum Lp] i32 (strictly increasing within a tracklet), the same for G ground-truth tracklets, all on the device ->
    [P, G] f32: the largest one-to-one IoU over the common frames, 0 without one.  One launch."""
    L.require_device(pd_boxes, pd_offsets, pd_frames, gt_boxes, gt_offsets, gt_frames)
    p, g = pd_offsets.numel() - 1, gt_offsets.numel() - 1
    pb, gb = pd_boxes[:, :7].contiguous().float(), gt_boxes[:, :7].contiguous().float()
    po, pf, go, gf = (t.contiguous().to(torch.int32) for t in (pd_offsets, pd_frames, gt_offsets, gt_frames))
    if pf.numel() != pb.size(0) or gf.numel() != gb.size(0):
        raise L.OcoccError('max_iou_packed: one frame index per box')
    out = torch.zeros((p, g), dtype=torch.float32, device=pb.device)
    L.check(L.lib.ococc_tracklet_max_iou_f32(L.ptr(pb), L.ptr(po), L.ptr(pf), p, L.ptr(gb), L.ptr(go), L.ptr(gf), g,
                                             L.ptr(out), L.stream()), 'tracklet_max_iou')
    return out


def frame_indices(ts_list, ts2frame):
    """timestamps of one tracklet -> their indices in the segment's sorted timestamp list; strictly increasing, which is
    what LiDARTracklet.freeze asserts of the timestamps (the kernel's binary search relies on it)"""
    out = [ts2frame[ts] for ts in ts_list]
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError('tracklet timestamps are not strictly increasing')
    return out


def pack_tracklets(tracklets, ts2frame):
    """host side of max_iou_packed: (boxes [sum L, 7] f32, offsets [n + 1] i32, frames [sum L] i32), CPU tensors"""
    offsets, frames = [0], []
    for t in tracklets:
        frames += frame_indices(t.ts_list, ts2frame)
        offsets.append(len(frames))
    boxes = torch.cat([t.boxes[:, :7].float() for t in tracklets], 0) if len(tracklets) else torch.zeros((0, 7))
    return boxes, torch.tensor(offsets, dtype=torch.int32), torch.tensor(frames, dtype=torch.int32)


def segment_ts2frame(*tracklet_lists):
    stamps = sorted({ts for trks in tracklet_lists for t in trks for ts in t.ts_list})
    return {ts: i for i, ts in enumerate(stamps)}


def tracklet_max_iou(pd_tracklets, gt_tracklets):
    """LiDARTracklet.max_iou (lidar_tracklet.py:210-229) of every pair of tracklets of one segment -> [P, G] f32 device
    tensor.  The tracklets' boxes live on the device."""
    L.require_device(*[t.boxes for t in pd_tracklets], *[t.boxes for t in gt_tracklets])
    if len(pd_tracklets) == 0 or len(gt_tracklets) == 0:
        dev = (list(pd_tracklets) + list(gt_tracklets))[0].device if len(pd_tracklets) + len(gt_tracklets) else 'cpu'
        return torch.zeros((len(pd_tracklets), len(gt_tracklets)), dtype=torch.float32, device=dev)
    dev = pd_tracklets[0].device
    ts2frame = segment_ts2frame(pd_tracklets, gt_tracklets)
    pb, po, pf = pack_tracklets(pd_tracklets, ts2frame)
    gb, go, gf = pack_tracklets(gt_tracklets, ts2frame)
    return max_iou_packed(pb, po.to(dev), pf.to(dev), gb, go.to(dev), gf.to(dev))


# ------------------------------------------------------------------------------------------------ configuration
def load_config(config):
    """a YAML file of the reference's tools/ctrl/data_configs shape (or the mapping itself, with key ``name``) ->
    (mapping, config name: what the output files are named after)"""
    if isinstance(config, (str, os.PathLike)):
        import yaml
        with open(config, 'r') as f:
            cfg = yaml.safe_load(f)
        name = osp.basename(str(config)).split('.')[0]
    else:
        cfg = dict(config)
        name = cfg.get('name')
        if not name:
            raise KeyError("a config given as a mapping needs a 'name' (the YAML file's base name)")
    if cfg['split'] not in SPLITS:
        raise ValueError(f"split must be one of {SPLITS}, got {cfg['split']!r}")
    return cfg, name


def bin_path_for_split(cfg):
    return cfg[{'training': 'bin_path', 'val': 'val_bin_path', 'test': 'test_bin_path'}[cfg['split']]]


def velodyne_dir(cfg):
    """<mm_data_root>/<training | testing>/velodyne: training and val share the 'training' directory"""
    kitti_split = 'training' if cfg['split'] in ('training', 'val') else 'testing'
    return osp.join(cfg.get('mm_data_root', MM_DATA_ROOT), kitti_split, 'velodyne')


def output_paths(cfg, name):
    stem = osp.join(cfg['data_root'], f"{name}_{cfg['split']}")
    return dict(info=stem + '.pkl', database=stem + '_database', candidates=stem + '_gt_candidates.pkl')


def select_tracklets(cfg, tracklets):
    mode, size = cfg['selection']['mode'], cfg['selection']['size']
    if mode == 'random':
        return tracklets[::int(1 / size)]
    raise NotImplementedError(f'selection mode {mode!r}')


def enlarged_boxes(boxes, extra_width):
    """LiDARInstance3DBoxes.enlarged_box (lidar_box3d.py:269-282): sizes + 2e, bottom centre z - e; a box a negative e
    would turn inside out keeps its size"""
    out = boxes.clone()
    out[:, 3:6] += extra_width * 2
    out[:, 2] -= extra_width
    if extra_width < 0:
        bad = (out[:, 3:6] <= 0).any(1)
        out[bad] = boxes[bad]
    return out


def _check_process(process):
    if not 1 <= int(process) <= MAX_PROCESSES:
        raise ValueError(f'--process {process}: between 1 and {MAX_PROCESSES} processes may share the GPUs')
    return int(process)


def _device(device):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise L.OcoccError('tracklet data preparation runs on a ROCm device only (there is no CPU fallback)')
    return torch.device('cuda', torch.cuda.current_device())


def _run_workers(fn, process, payload, device):
    """segments dealt round-robin over ``process`` fresh spawned children (segment i to token i % process, device
    token % device_count); a child's exception is raised here.  process == 1 runs in this process."""
    if process == 1:
        return [fn(0, 1, payload, device)]
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(max_workers=process, mp_context=mp.get_context('spawn')) as pool:
        futures = [pool.submit(fn, token, process, payload, None if device is None else str(device)) for token in range(process)]
        return [f.result() for f in futures]


def _worker_device(token, device):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise L.OcoccError('tracklet data preparation runs on a ROCm device only (there is no CPU fallback)')
    torch.cuda.set_device(token % torch.cuda.device_count())
    return torch.device('cuda', torch.cuda.current_device())


# ------------------------------------------------------------------------------------------------ step 4: track input
def load_frame_index(mm_data_root):
    """idx2timestamp.pkl / idx2contextname.pkl -> ({timestamp: frame file index}, {segment: sorted timestamps})"""
    with open(osp.join(mm_data_root, 'idx2timestamp.pkl'), 'rb') as f:
        idx2ts = pickle.load(f)
    with open(osp.join(mm_data_root, 'idx2contextname.pkl'), 'rb') as f:
        idx2seg = pickle.load(f)
    ts2idx = {ts: idx for idx, ts in idx2ts.items()}
    seg_ts = defaultdict(list)
    for ts, seg in {idx2ts[idx]: seg for idx, seg in idx2seg.items()}.items():
        seg_ts[seg].append(ts)
    for v in seg_ts.values():
        v.sort()
    return ts2idx, dict(seg_ts)


def _crop_segment(trks, full_ts, ts2idx, pc_root, extra_width, device):
    """trks: [(boxes [L, 7] CPU tensor, ts_list)] of one segment -> per tracklet the list of per-frame [n, 6] arrays"""
    at = defaultdict(list)                       # timestamp -> [(tracklet, position in the tracklet)]
    for i, (_, ts_list) in enumerate(trks):
        for k, ts in enumerate(ts_list):
            at[ts].append((i, k))
    missing = set(at) - set(full_ts)
    if missing:
        raise KeyError(f'{len(missing)} tracklet timestamps have no frame in idx2timestamp.pkl (e.g. {sorted(missing)[0]})')
    pcs = [[None] * len(ts_list) for _, ts_list in trks]
    batch, batch_bytes = [], 0

    def flush():
        nonlocal batch, batch_bytes
        if not batch:
            return
        clouds = [pc for _, pc in batch]
        po = np.concatenate([[0], np.cumsum([len(pc) for pc in clouds])])
        owners = [at[ts] for ts, _ in batch]
        bo = np.concatenate([[0], np.cumsum([len(o) for o in owners])])
        boxes = torch.stack([trks[i][0][k, :7].float() for o in owners for i, k in o], 0)
        points = torch.from_numpy(np.concatenate(clouds, 0)).to(device)
        counts, out_index = crop_frames_packed(points, po.tolist(), enlarged_boxes(boxes, extra_width).to(device), bo.tolist())
        base = torch.from_numpy(np.repeat(po[:-1], np.diff(bo)))          # per box: first row of its frame
        rows = points[out_index + torch.repeat_interleave(base, counts).to(device)].cpu().numpy()   # one gather, one copy
        scan = np.concatenate([[0], np.cumsum(counts.numpy())])
        for b, (i, k) in enumerate(ik for o in owners for ik in o):
            pcs[i][k] = rows[scan[b]:scan[b + 1]].copy()
        batch, batch_bytes = [], 0

    for ts in full_ts:
        if ts not in at:
            continue
        pc = np.fromfile(osp.join(pc_root, f'{ts2idx[ts]}.bin'), dtype=np.float32).reshape(-1, 6)
        if batch and (batch_bytes + pc.nbytes > CROP_BATCH_BYTES or len(batch) >= 65535):
            flush()
        batch.append((ts, pc))
        batch_bytes += pc.nbytes
    flush()
    return pcs


def _track_input_worker(token, process, payload, device):
    device = _worker_device(token, device)
    out = {}
    for seg_idx, (seg, trks) in enumerate(payload['segments']):
        if seg_idx % process != token:
            continue
        pcs = _crop_segment([(torch.from_numpy(b), ts) for _, b, ts in trks], payload['seg_ts'].get(seg, []), payload['ts2idx'],
                            payload['pc_root'], payload['extra_width'], device)
        for (tid, _, _), pc in zip(trks, pcs):
            arr = np.empty(len(pc), dtype=object)
            for i, p in enumerate(pc):
                arr[i] = p
            with open(osp.join(payload['save_dir'], f'{seg}--{tid}.npy'), 'wb') as fw:
                np.save(fw, arr, allow_pickle=True)
        out[seg] = [[len(p) for p in pc] for pc in pcs]
    return out


def generate_track_input(config, process=1, device=None):
    """tools/ctrl/generate_track_input.py as a function: detections (.bin) -> tracklets -> the points inside every
    enlarged box -> <name>_<split>_database/*.npy and <name>_<split>.pkl.  Returns the path of the .pkl."""
    process = _check_process(process)
    cfg, name = load_config(config)
    paths = output_paths(cfg, name)
    if not cfg['exist_ok'] and osp.exists(paths['info']):
        raise FileExistsError(f"{paths['info']} exists and exist_ok is false")
    print(f"Point clouds will be saved to {paths['database']}")
    print(f"Pickled Info will be saved to {paths['info']}")
    tracklets = waymo_io.generate_tracklets(waymo_io.read_bin(bin_path_for_split(cfg)))
    if cfg['split'] == 'training':
        tracklets = select_tracklets(cfg, tracklets)
    ts2idx, seg_ts = load_frame_index(cfg.get('mm_data_root', MM_DATA_ROOT))
    os.makedirs(paths['database'], exist_ok=bool(cfg['exist_ok']))
    by_seg = defaultdict(list)
    for t in tracklets:
        by_seg[t.segment_name].append(t)
    payload = dict(segments=[(seg, [(t.id, t.boxes.numpy(), t.ts_list) for t in trks]) for seg, trks in by_seg.items()],
                   seg_ts=seg_ts, ts2idx=ts2idx, pc_root=velodyne_dir(cfg), extra_width=cfg['box']['extra_width'],
                   save_dir=paths['database'])
    num_pts = {}
    for part in _run_workers(_track_input_worker, process, payload, device if process > 1 else _device(device)):
        num_pts.update(part)
    for seg, trks in by_seg.items():
        assert len(num_pts[seg]) == len(trks)
        for t, n in zip(trks, num_pts[seg]):
            t.num_pts_in_boxes = n
    with open(paths['info'], 'wb') as fw:
        pickle.dump([t.to_dump_format() for t in tracklets], fw)
    print(f"Tracklets saved to {paths['info']}")
    return paths['info']


# ------------------------------------------------------------------------------------------------ step 5: candidates
def segment_candidates(pd_tracklets, gt_tracklets, thresh, device):
    """per predicted tracklet the positions (GT order) of the GT tracklets with max IoU > thresh: one launch, one read-back"""
    if not pd_tracklets or not gt_tracklets:
        return [[] for _ in pd_tracklets]
    ts2frame = segment_ts2frame(pd_tracklets, gt_tracklets)
    packed = [x.to(device) for trks in (pd_tracklets, gt_tracklets) for x in pack_tracklets(trks, ts2frame)]
    affinity = max_iou_packed(*packed).cpu().numpy()
    return [np.nonzero(row > thresh)[0].tolist() for row in affinity]


def _candidates_worker(token, process, payload, device):
    device = _worker_device(token, device)
    out = {}
    for seg_idx, (seg, pd) in enumerate(payload['pd']):
        if seg_idx % process != token or seg not in payload['gt']:
            continue
        mk = lambda rows: [Tracklet(torch.from_numpy(b), ts) for b, ts in rows]
        out[seg] = segment_candidates(mk(pd), mk(payload['gt'][seg]), payload['thresh'], device)
    return out


def candidate_stats(tracklets, candidates_list):
    """the two lines of generate_candidates.py:stats"""
    unmatched = [t for t, c in zip(tracklets, candidates_list) if len(c) == 0]
    print(f'Tracklet FP rate: {len(unmatched) / max(len(tracklets), 1)}')
    print(f'Box FP rate: {sum(len(t) for t in unmatched) / max(sum(len(t) for t in tracklets), 1)}')


def generate_candidates(config, gt_bin_path='./data/waymo/waymo_format/train_gt.bin', process=1, device=None):
    """tools/ctrl/generate_candidates.py as a function: <name>_<split>.pkl + the ground-truth .bin ->
    <name>_<split>_gt_candidates.pkl (per predicted tracklet, in their order, the dump tuples of the GT tracklets of its
    segment with max IoU > candidate.affinity_thresh, in GT order).  Returns the path written."""
    process = _check_process(process)
    cfg, name = load_config(config)
    paths = output_paths(cfg, name)
    print(f"Results will be saved to {paths['candidates']}")
    if cfg['split'] == 'val':
        gt_bin_path = gt_bin_path.replace('train_gt.bin', 'gt.bin')
    gt = waymo_io.generate_tracklets(waymo_io.read_bin(gt_bin_path), set(cfg['type']))
    with open(paths['info'], 'rb') as fr:
        pd = [Tracklet.from_dump_format(e) for e in pickle.load(fr)]
    gt_by_seg, pd_by_seg = defaultdict(list), defaultdict(list)
    for t in gt:
        gt_by_seg[t.segment_name].append(t)
    for i, t in enumerate(pd):
        pd_by_seg[t.segment_name].append(i)
    rows = lambda trks: [(t.boxes.numpy(), t.ts_list) for t in trks]   # (plain arrays: they cross to spawned children)
    payload = dict(pd=[(seg, rows([pd[i] for i in idx])) for seg, idx in pd_by_seg.items()],
                   gt={seg: rows(trks) for seg, trks in gt_by_seg.items()}, thresh=cfg['candidate']['affinity_thresh'])
    picked = {}
    for part in _run_workers(_candidates_worker, process, payload, device if process > 1 else _device(device)):
        picked.update(part)
    out = [[] for _ in pd]
    for seg, idx in pd_by_seg.items():
        if seg not in picked:
            continue
        dumps = [t.to_dump_format() for t in gt_by_seg[seg]]
        for i, cand in zip(idx, picked[seg]):
            out[i] = [dumps[j] for j in cand]
    scored = sum(len(idx) for seg, idx in pd_by_seg.items() if seg in picked)
    print(f'Average candidates per trk {sum(len(c) for c in out) / max(scored, 1)}')
    candidate_stats(pd, out)
    with open(paths['candidates'], 'wb') as fw:
        pickle.dump(out, fw)
    return paths['candidates']


# ------------------------------------------------------------------------------------------------ track extension
MAX_FIRST_GAP_MICROS = 500_000    # extend / extend_all give up when the first two boxes are further apart than this
EXTEND_KEYS = ('bin_path', 'direction', 'extend_length', 'min_length_to_extend', 'score_multiplier', 'velo_window_size')


def load_extend_config(config):
    """a YAML file of the reference's tools/ctrl/data_configs/extend.yaml shape (or the mapping itself, with key
    ``name``) -> (mapping, config name).  Optional keys: extend_all, min_length_to_extend_all, mm_data_root,
    poses_path (default <mm_data_root>/poses.pkl)."""
    if isinstance(config, (str, os.PathLike)):
        import yaml
        with open(config, 'r') as f:
            cfg = yaml.safe_load(f)
        name = osp.basename(str(config)).split('.')[0]
    else:
        cfg = dict(config)
        name = cfg.get('name')
        if not name:
            raise KeyError("a config given as a mapping needs a 'name' (the YAML file's base name)")
    missing = [k for k in EXTEND_KEYS if k not in cfg]
    if missing:
        raise KeyError(f'extend config misses {missing}')
    if cfg['direction'] not in ('forward', 'backward'):
        raise ValueError(f"direction must be 'forward' or 'backward', got {cfg['direction']!r}")
    if cfg['direction'] == 'forward':
        raise NotImplementedError('direction: forward (LiDARTracklet.extend raises for it too; the tracker extends forward)')
    if cfg.get('extend_all', False) and 'min_length_to_extend_all' not in cfg:
        raise KeyError('extend_all needs min_length_to_extend_all')
    if int(cfg['extend_length']) < 0 or int(cfg['velo_window_size']) < 1:
        raise ValueError('extend_length must not be negative and velo_window_size at least 1')
    return cfg, name


def plan_extension(offsets, frames, segments, seg_ts, extend_length, min_length, extend_all=False, min_length_all=0,
                   direction='backward'):
    """Who is extended and by how much -- the integer part of LiDARTracklet.extend / extend_all and of the choice
    between them (tools/ctrl/extend_tracks.py:171-188), on the host.  offsets [n + 1], frames [sum L] (index of every
    box in its segment's sorted timestamps), segments [n], seg_ts: per segment its sorted timestamps (microseconds)
    -> (num_back [n], num_fwd [n], out_offsets [n + 1]) int32 arrays.

    extend_all is taken when set and L > min_length_all, else plain extend.  Not extended: fewer boxes than the
    minimum length of the branch taken; a first gap ts[1] - ts[0] above 500 000 microseconds (for extend_all this
    cancels the forward part too) -- the reference tests delta_t > 0.5 on float32 seconds, which for integer
    microseconds is this integer test (0.5 is exact in float32 and rounding is monotone); a tracklet of ONE box, where
    the reference would raise on ts_in_sec[1], is never extended.  backward: min(extend_length, first frame index)
    frames; extend_all: every frame of the segment before the first and after the last box."""
    if direction != 'backward':
        raise NotImplementedError(f'direction {direction!r}: only backward extension exists (as upstream)')
    offsets, frames, segments = (np.asarray(v, dtype=np.int64) for v in (offsets, frames, segments))
    n = len(segments)
    back, fwd = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for t in range(n):
        lo, hi = offsets[t], offsets[t + 1]
        length, stamps = hi - lo, seg_ts[segments[t]]
        use_all = bool(extend_all) and length > min_length_all
        if length < (min_length_all if use_all else min_length) or length < 2:
            continue
        if stamps[frames[lo + 1]] - stamps[frames[lo]] > MAX_FIRST_GAP_MICROS:
            continue
        if use_all:
            back[t], fwd[t] = frames[lo], len(stamps) - 1 - frames[hi - 1]
        else:
            back[t] = min(int(extend_length), frames[lo])
    out_offsets = np.zeros(n + 1, np.int32)
    np.cumsum(np.diff(offsets) + back + fwd, out=out_offsets[1:])
    return back, fwd, out_offsets


def extend_tracks_packed(boxes, offsets, frames, segments, scores, poses, timestamps, seg_offsets, num_back, num_fwd,
                         out_offsets, score_multiplier, velo_window_size):
    """The boxes of n tracklets back to back [sum L, 7] f32 (each in its frame's ego frame) with their scores [sum L]
    f64, the poses [sum T, 16] f32 (ego -> world) and timestamps [sum T] int64 of all segments back to back, on the
    device; offsets [n + 1], frames [sum L], segments [n], seg_offsets [S + 1] and the plan of plan_extension as HOST
    integer sequences -> (boxes [sum L', 7] f32 in each output frame's own ego frame, scores [sum L'] f64, frame indices
    [sum L'] i32) on the device.  One launch, no read-back between the plan and the launch."""
    L.require_device(boxes, scores, poses, timestamps)
    if boxes.dim() != 2 or boxes.size(1) < 7 or boxes.dtype != torch.float32:
        raise L.OcoccError(f'boxes must be [N, >= 7] float32, got {tuple(boxes.shape)} {boxes.dtype}')
    if scores.dtype != torch.float64 or scores.numel() != boxes.size(0):
        raise L.OcoccError('extend_tracks: one float64 score per box')
    if timestamps.dtype != torch.int64 or poses.dtype != torch.float32 or poses.numel() != timestamps.numel() * 16:
        raise L.OcoccError('extend_tracks: poses [T, 16] float32 (or [T, 4, 4]) and timestamps [T] int64')
    off, fr, seg, so, nb, nf, oo = (np.asarray(v, dtype=np.int64).reshape(-1) for v in
                                   (offsets, frames, segments, seg_offsets, num_back, num_fwd, out_offsets))
    n, total, num_frames = len(seg), boxes.size(0), timestamps.numel()
    if len(off) != n + 1 or len(nb) != n or len(nf) != n or len(oo) != n + 1 or len(fr) != total or len(so) < 1:
        raise L.OcoccError('extend_tracks: table lengths do not fit the number of tracklets / boxes')
    lens = np.diff(off)
    if off[0] != 0 or off[-1] != total or (lens < 1).any() or so[0] != 0 or so[-1] != num_frames or (np.diff(so) < 0).any() \
            or oo[0] != 0 or (np.diff(oo) != lens + nb + nf).any() or (nb < 0).any() or (nf < 0).any() \
            or (n and (seg.min() < 0 or seg.max() >= len(so) - 1)) or oo[-1] >= 2 ** 31:
        raise L.OcoccError('extend_tracks: offsets must start at 0 and end at the row counts, every tracklet needs a box, '
                           'and out_offsets must be the running sum of num_back + length + num_fwd')
    if n:
        frames_of = np.diff(so)[seg]
        inner = np.ones(total, bool)
        inner[off[:-1]] = False
        if (fr < 0).any() or (fr >= np.repeat(frames_of, lens)).any() or (np.diff(fr, prepend=-1)[inner] <= 0).any():
            raise L.OcoccError('extend_tracks: frame indices must lie in their segment and increase within a tracklet')
        if (fr[off[:-1]] - nb < 0).any() or (fr[off[1:] - 1] + nf >= frames_of).any():
            raise L.OcoccError('extend_tracks: the plan leaves the segment')
    if not int(velo_window_size) >= 1:
        raise L.OcoccError('extend_tracks: velo_window_size must be at least 1')
    dev = boxes.device
    num_out = int(oo[-1]) if n else 0
    out_boxes = torch.empty((num_out, 7), dtype=torch.float32, device=dev)
    out_scores = torch.empty((num_out,), dtype=torch.float64, device=dev)
    out_frames = torch.empty((num_out,), dtype=torch.int32, device=dev)
    if n == 0:
        return out_boxes, out_scores, out_frames
    tables = [off, fr, seg, so, nb, nf, oo]
    flat = torch.from_numpy(np.concatenate(tables).astype(np.int32)).to(dev)              # one upload
    d_off, d_fr, d_seg, d_so, d_nb, d_nf, d_oo = flat.split([len(v) for v in tables])
    boxes7 = boxes[:, :7].contiguous()
    L.check(L.lib.ococc_track_extend_f64(L.ptr(boxes7), L.ptr(d_off), L.ptr(d_fr), L.ptr(d_seg), L.ptr(scores.contiguous()), n,
                                         total, L.ptr(poses.contiguous()), L.ptr(timestamps.contiguous()), L.ptr(d_so),
                                         len(so) - 1, num_frames, L.ptr(d_nb), L.ptr(d_nf), L.ptr(d_oo), num_out,
                                         float(score_multiplier), int(velo_window_size), L.ptr(out_boxes), L.ptr(out_scores),
                                         L.ptr(out_frames), L.stream()), 'track_extend')
    return out_boxes, out_scores, out_frames


def pack_for_extension(tracklets, seg_ts, ts2pose):
    """host side of extend_tracks_packed: tracklets (ego-frame boxes, ``segment_name``) -> dict of CPU tensors / arrays
    (boxes, scores, offsets, frames, segments, poses, timestamps, seg_offsets, names: the segments in table order)"""
    names, seg_of, ts2frame_of = [], {}, {}
    offsets, frames, segments = [0], [], []
    for t in tracklets:
        if t.segment_name not in seg_of:
            if t.segment_name not in seg_ts:
                raise KeyError(f'segment {t.segment_name!r} has no frames in idx2contextname.pkl')
            seg_of[t.segment_name] = len(names)
            names.append(t.segment_name)
            ts2frame_of[t.segment_name] = {ts: i for i, ts in enumerate(seg_ts[t.segment_name])}
        ts2frame = ts2frame_of[t.segment_name]
        missing = [ts for ts in t.ts_list if ts not in ts2frame]
        if missing:
            raise KeyError(f'tracklet {t.id!r}: timestamp {missing[0]} is not a frame of {t.segment_name!r}')
        frames += frame_indices(t.ts_list, ts2frame)
        offsets.append(len(frames))
        segments.append(seg_of[t.segment_name])
    stamps = [ts for s in names for ts in seg_ts[s]]
    lost = [ts for ts in stamps if ts not in ts2pose]
    if lost:
        raise KeyError(f'{len(lost)} frames have no pose in poses.pkl (e.g. {lost[0]})')
    poses = np.stack([np.asarray(ts2pose[ts], dtype=np.float32).reshape(16) for ts in stamps], 0) if stamps else np.zeros((0, 16), np.float32)
    boxes = torch.cat([t.boxes[:, :7].float() for t in tracklets], 0) if len(tracklets) else torch.zeros((0, 7))
    scores = torch.cat([t.scores.double() for t in tracklets], 0) if len(tracklets) else torch.zeros((0,), dtype=torch.float64)
    return dict(boxes=boxes, scores=scores, offsets=np.asarray(offsets), frames=np.asarray(frames, dtype=np.int64),
                segments=np.asarray(segments, dtype=np.int64), poses=torch.from_numpy(poses),
                timestamps=torch.tensor(stamps, dtype=torch.int64),
                seg_offsets=np.concatenate([[0], np.cumsum([len(seg_ts[s]) for s in names])]).astype(np.int64), names=names)


def extend_tracks(config, device=None):
    """tools/ctrl/extend_tracks.py as a function: the tracker's result (.bin) -> every tracklet extended backward by a
    constant-velocity model (over the whole segment with ``extend_all``) -> <bin stem>_<config name>.bin, objects in the
    reference's order (tracklets in order of first appearance, frames ascending), the tracklet's Waymo type written as
    it is, the score a 32-bit float on the wire.  The frame lists come from idx2timestamp.pkl / idx2contextname.pkl
    (load_frame_index), the poses from ``poses_path`` (default <mm_data_root>/poses.pkl).  All tracklets of the file
    are one launch.  Returns the path written."""
    cfg, name = load_extend_config(config)
    device = _device(device)
    save_path = osp.splitext(cfg['bin_path'])[0] + f'_{name}.bin'
    print(f'Result will be saved to {save_path}')
    objects = waymo_io.read_bin(cfg['bin_path'])
    print(f'Got {len(objects)} objects before extending')
    tracklets = waymo_io.generate_tracklets(objects)
    mm_root = cfg.get('mm_data_root', MM_DATA_ROOT)
    _, seg_ts = load_frame_index(mm_root)
    with open(cfg.get('poses_path') or osp.join(mm_root, 'poses.pkl'), 'rb') as fr:
        ts2pose = pickle.load(fr)
    pk = pack_for_extension(tracklets, seg_ts, ts2pose)
    use_all = bool(cfg.get('extend_all', False))
    print(f'Extend all timestamps? {use_all}')
    back, fwd, out_offsets = plan_extension(pk['offsets'], pk['frames'], pk['segments'], [seg_ts[s] for s in pk['names']],
                                            cfg['extend_length'], cfg['min_length_to_extend'], use_all,
                                            cfg.get('min_length_to_extend_all', 0), cfg['direction'])
    boxes, scores, frames = extend_tracks_packed(pk['boxes'].to(device), pk['offsets'], pk['frames'], pk['segments'],
                                                 pk['scores'].to(device), pk['poses'].to(device), pk['timestamps'].to(device),
                                                 pk['seg_offsets'], back, fwd, out_offsets, cfg['score_multiplier'],
                                                 cfg['velo_window_size'])
    boxes, scores, frames = boxes.cpu().numpy(), scores.cpu().numpy(), frames.cpu().numpy()
    chunks = []
    for k, t in enumerate(tracklets):
        assert t.type in (1, 2, 4) and isinstance(t.id, str)
        stamps = seg_ts[t.segment_name]
        for q in range(out_offsets[k], out_offsets[k + 1]):
            chunks.append(waymo_io._f_bytes(1, waymo_io.lidar2waymo_box(boxes[q], scores[q], t.type, t.segment_name,
                                                                         stamps[frames[q]], t.id)))
    with open(save_path, 'wb') as f:
        f.write(b''.join(chunks))
    print(f'Convert finished, got {len(chunks)} objects. Saved to {save_path}')
    return save_path


# ------------------------------------------------------------------------------------------------ empty-box removal
BOTTOM_LIFT = {'vehicle': 0.2, 'pedestrian': 0.1, 'cyclist': 0.1}     # tools/ctrl/remove_empty.py:155-160
KITTI_SPLIT = {'training': 'training', 'val': 'training', 'validation': 'training', 'test': 'testing', 'testing': 'testing'}


def nonempty_frames_packed(points, point_offsets, boxes, box_offsets):
    """Arguments as crop_frames_packed -> flags [B] int32 on the device: 1 where crop_frames_packed would count at
    least one point in the box (the same membership arithmetic).  One launch, no workspace, no read-back."""
    L.require_device(points, boxes)
    if points.dim() != 2 or points.size(1) < 3 or points.dtype != torch.float32:
        raise L.OcoccError(f'points must be [N, >= 3] float32, got {tuple(points.shape)} {points.dtype}')
    po, bo = [int(v) for v in point_offsets], [int(v) for v in box_offsets]
    frames = len(po) - 1
    if len(bo) != frames + 1 or frames < 0 or po[0] != 0 or bo[0] != 0 or po[-1] != points.size(0) or bo[-1] != boxes.size(0) \
            or any(b < a for a, b in zip(po, po[1:])) or any(b < a for a, b in zip(bo, bo[1:])):
        raise L.OcoccError('nonempty_frames: offsets must start at 0, not decrease and end at the row counts')
    dev = points.device
    points = points.contiguous()
    boxes = boxes[:, :7].contiguous().float()
    n, b = points.size(0), boxes.size(0)
    flags = torch.zeros((b,), dtype=torch.int32, device=dev)
    if b == 0 or n == 0 or frames == 0:
        return flags
    max_pts = max(y - x for x, y in zip(po, po[1:]))
    offs = torch.tensor(po + bo, dtype=torch.int64).to(dev)
    L.check(L.lib.ococc_tracklet_nonempty(L.ptr(points), n, points.size(1), L.ptr(offs[:frames + 1]), L.ptr(boxes), b,
                                          L.ptr(offs[frames + 1:]), frames, max_pts, L.ptr(flags), L.stream()),
            'tracklet_nonempty')
    return flags


def lifted_lidar_boxes(objects, bottom_lift):
    """records of read_bin -> [n, 7] f32 boxes as bin2lidarboxes + LiDARInstance3DBoxes(origin=(0.5, 0.5, 0.5)) make
    them (tools/ctrl/utils.py:68-95, 115-144; remove_empty.py:83-88): bottom centre, (width, length, height) kept in
    the file's order, yaw = -heading - pi/2 wrapped into [-pi, pi], float32 from there on, then the bottom lifted by
    bottom_lift * height"""
    rows = np.zeros((len(objects), 7), np.float64)
    for i, o in enumerate(objects):
        heading = -o['heading'] - 0.5 * np.pi
        while heading < -np.pi:
            heading += 2 * np.pi
        while heading > np.pi:
            heading -= 2 * np.pi
        rows[i] = [o['center_x'], o['center_y'], o['center_z'], o['width'], o['length'], o['height'], heading]
    boxes = torch.from_numpy(rows).float()
    boxes[:, 2] += boxes[:, 5] * -0.5
    boxes[:, 2] += boxes[:, 5] * bottom_lift
    return boxes


def _nonempty_worker(token, process, payload, device):
    device = _worker_device(token, device)
    out, batch, batch_bytes = {}, [], 0

    def flush():
        nonlocal batch, batch_bytes
        if not batch:
            return
        po = np.concatenate([[0], np.cumsum([len(pc) for _, pc, _ in batch])])
        bo = np.concatenate([[0], np.cumsum([len(b) for _, _, b in batch])])
        points = torch.from_numpy(np.concatenate([pc for _, pc, _ in batch], 0)).to(device)
        boxes = torch.from_numpy(np.concatenate([b for _, _, b in batch], 0)).to(device)
        flags = nonempty_frames_packed(points, po.tolist(), boxes, bo.tolist()).cpu().numpy()   # one read-back per batch
        for i, (k, _, _) in enumerate(batch):
            out[k] = flags[bo[i]:bo[i + 1]].astype(bool)
        batch, batch_bytes = [], 0

    for k, (ts, boxes) in enumerate(payload['frames']):
        if k % process != token:
            continue
        if ts not in payload['ts2idx']:
            raise KeyError(f'timestamp {ts} has no frame in idx2timestamp.pkl')
        pc = np.fromfile(osp.join(payload['pc_root'], f"{payload['ts2idx'][ts]}.bin"), dtype=np.float32).reshape(-1, 6)
        if batch and (batch_bytes + pc.nbytes > CROP_BATCH_BYTES or len(batch) >= 65535):
            flush()
        batch.append((k, pc, boxes))
        batch_bytes += pc.nbytes
    flush()
    return out


def remove_empty(bin_path, split, type='vehicle', process=1, gt_bin=None, device=None, mm_data_root=None, extra_hw=0.0):
    """tools/ctrl/remove_empty.py as a function: every box of ``bin_path`` that holds no lidar point of its frame, after
    its bottom was lifted by 0.2 (vehicle) / 0.1 (pedestrian, cyclist) of its height, is dropped; the kept objects are
    written UNCHANGED (waymo_io.write_objects) to <stem>_wo_empty_right.bin, frames in the file's order of first
    appearance and boxes in file order -- whatever ``process`` is (the reference's order depends on how its worker
    processes are scheduled).  split: 'training' (also 'val') or 'testing' ('test'), the velodyne directory under
    ``mm_data_root``.  A batch of frames is one launch and one read-back.  With ``gt_bin`` the waymo_native table of the
    result is printed and written next to it (<stem>_wo_empty_right.txt), in place of the reference's call of the
    compiled Waymo tool.  Returns the path written."""
    process = _check_process(process)
    if type not in BOTTOM_LIFT:
        raise NotImplementedError(f'type {type!r}: one of {sorted(BOTTOM_LIFT)}')
    if split not in KITTI_SPLIT:
        raise ValueError(f'split must be one of {sorted(KITTI_SPLIT)}, got {split!r}')
    if extra_hw:
        raise NotImplementedError('extra_hw other than 0 (enlarged_box_hw) is not built; the reference always runs with 0')
    mm_root = mm_data_root or MM_DATA_ROOT
    save_path = osp.join(osp.dirname(bin_path), osp.basename(bin_path).split('.')[0] + '_wo_empty_right.bin')
    print(f'Results will be saved to {save_path}')
    objects = waymo_io.read_bin(bin_path)
    ts2idx, _ = load_frame_index(mm_root)
    boxes = lifted_lidar_boxes(objects, BOTTOM_LIFT[type]).numpy()
    rows_of = defaultdict(list)                                  # timestamp -> object rows, file order
    for i, o in enumerate(objects):
        rows_of[o['frame_timestamp_micros']].append(i)
    payload = dict(frames=[(ts, boxes[rows]) for ts, rows in rows_of.items()], ts2idx=ts2idx,
                   pc_root=osp.join(mm_root, KITTI_SPLIT[split], 'velodyne'))
    flags = {}
    for part in _run_workers(_nonempty_worker, process, payload, device if process > 1 else _device(device)):
        flags.update(part)
    keep = [objects[i] for k, rows in enumerate(rows_of.values()) for i, f in zip(rows, flags[k]) if f]
    print(f'Num objects after remove: {len(keep)}')
    waymo_io.write_objects(keep, save_path)
    if gt_bin is not None:
        from . import waymo_metrics
        waymo_metrics.evaluate_files(save_path, gt_bin, txt_path=save_path.replace('.bin', '.txt'))
    return save_path
