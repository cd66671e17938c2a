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
one fill launch, a segment's P x G affinity matrix one launch and one read-back."""
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
