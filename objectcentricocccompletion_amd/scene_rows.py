"""The first stage of online inference from sensor frames: one scene cloud, in the ego frame it was taken in, and the
tracker's boxes of that frame -> the step rows TrackletRoIHeadOCC.simple_test_step takes (csrc/scene_rows.hip).

Offline, the same rows come out of a chain of passes: the crop into the enlarged boxes
(tools/ctrl/generate_track_input.py:84-99, csrc/tracklet_crop.hip), the per-tracklet .npy files and their cap of 1024
points per frame (LoadTrackletPoints), the move into the tracklet's fixed frame (TrackletPoseTransform), the decoration
with yaw / 3.1415, size / 10 and score (PointDecoration), the range filter (PointsRangeFilter) and the row index.  Here a
frame is one count launch, one read-back of the counts and one fill launch that writes the rows (scene_step_rows); the
frames of a chunked step -- several clouds, a row per (tracklet, frame) -- are one count launch, one read-back and one
fill launch together (scene_steps_rows).

Two deviations from the offline chain, both because a step must be reproducible: where LoadTrackletPoints draws a random
subset of max_points points, the kernel takes an even pick in the cloud's order (point j of m is kept iff
(j+1)*cap//m > j*cap//m), and there is no PointShuffle (the rows keep the cloud's order)."""
import numpy as np
import torch

from . import _lib as L
from .ctrl_prep import enlarged_boxes

EXTRA_WIDTH = 1.0            # box.extra_width of tools/ctrl/data_configs/*.yaml: the margin generate_track_input crops with
ROW_FEAT_DIM = 5             # yaw / 3.1415, w / 10, l / 10, h / 10, score


def even_pick(m, cap):
    """The cap's rule on the host: [(j, place)] of the members of a box of m points that survive a cap of ``cap`` rows, in
    Python ints -- what ococc_scene_rows_fill computes in int64."""
    if cap <= 0 or m <= cap:
        return [(j, j) for j in range(m)]
    return [(j, j * cap // m) for j in range(m) if (j + 1) * cap // m > j * cap // m]


def decoration(boxes, scores):
    """PointDecoration's yaw, size and score columns of n boxes as one [n, 5] f32 tensor, with its own expressions: the yaw
    divided in double precision (``float(box[6]) / 3.1415``), the sizes in f32 (``boxes[:, 3:6] / 10``), the score as it
    is.  The divisors are tensors: ATen turns a division by a host scalar into a multiplication by its reciprocal."""
    dev = boxes.device
    yaw = (boxes[:, 6].double() / L.const_tensor([3.1415], dev, torch.float64)).float()
    size = boxes[:, 3:6].float() / L.const_tensor([10.0], dev)
    return torch.cat([yaw[:, None], size, scores.float().reshape(-1, 1)], 1)


def _check_rows(points, boxes, scores, transforms, attr_dims, point_cloud_range, max_points, deco_boxes):
    """the shape and value checks of scene_step_rows / scene_steps_rows (no device needed) -> (n, N, cap)"""
    if points.dim() != 2 or points.dtype != torch.float32 or points.size(1) < 3 + int(attr_dims) or attr_dims < 0:
        raise L.OcoccError(f'points must be [N, >= 3 + attr_dims = {3 + int(attr_dims)}] float32, got {tuple(points.shape)} '
                           f'{points.dtype}')
    if boxes.dim() != 2 or boxes.size(1) < 7:
        raise L.OcoccError(f'boxes must be [n, 7], got {tuple(boxes.shape)}')
    n, N = boxes.size(0), points.size(0)
    if scores.numel() != n or (deco_boxes is not None and tuple(deco_boxes.shape[:1]) != (n,)):
        raise L.OcoccError(f'{scores.numel()} scores (and deco_boxes) for {n} boxes')
    if transforms is not None and (transforms.numel() != n * 12 or transforms.dtype != torch.float32):
        raise L.OcoccError(f'transforms must be [n, 12] float32, got {tuple(transforms.shape)} {transforms.dtype}')
    if point_cloud_range is not None and len(point_cloud_range) != 6:
        raise L.OcoccError('point_cloud_range is (x0, y0, z0, x1, y1, z1)')
    cap = int(max_points)
    if cap > 2 ** 31 - 1:
        raise L.OcoccError('max_points is at most 2**31 - 1')
    return n, N, cap


def _row_inputs(points, boxes, scores, transforms, extra_width, point_cloud_range, deco_boxes):
    """what both operators hand the kernels, from checked arguments: the contiguous cloud, the enlarged crop boxes, the
    decoration [n, 5], the matrices [n, 12] or None, the range as a host array or None"""
    n = boxes.size(0)
    if transforms is not None:
        transforms = transforms.reshape(n, 12).contiguous()
    rng = None if point_cloud_range is None else L.f6(point_cloud_range)
    boxes = boxes[:, :7].contiguous().float()
    crop = enlarged_boxes(boxes, extra_width)
    row_feats = decoration(boxes if deco_boxes is None else deco_boxes[:, :7].float(), scores).contiguous()
    return points.contiguous(), crop, row_feats, transforms, rng


def scene_step_rows(points, boxes, scores, transforms=None, extra_width=EXTRA_WIDTH, attr_dims=2, point_cloud_range=None,
                    max_points=-1, deco_boxes=None):
    """points [N, >= 3 + attr_dims] f32: the scene cloud of one sensor frame; boxes [n, 7] f32 (x, y, z_bottom, w, l, h,
    yaw): the proposals in the cloud's frame, scores [n].  Row b takes the points inside ``enlarged_boxes(boxes,
    extra_width)[b]`` (a point may be in several rows), in the cloud's order.

    transforms [n, 12] f32 (or [n, 3, 4]): per row the row-major 3x4 matrix its points go through (f32 fused
    multiply-adds); None leaves them.  With transforms the decoration is taken from ``deco_boxes`` [n, 7], the boxes in
    the TARGET frame (default: ``boxes``, for a caller that passes none or has them there already).
    point_cloud_range (x0, y0, z0, x1, y1, z1): only points whose written xyz lies strictly inside are rows.
    max_points = cap > 0: at most cap rows per box, an even pick in the cloud's order (even_pick).

    Returns (xyz [M, 3] f32, feats [M, attr_dims + 5] f32 = the point's columns 3 : 3 + attr_dims, then yaw / 3.1415,
    size / 10, score of its row, row [M] i64, counts [n] i64 on the HOST: the members per box BEFORE the cap).  Rows are
    sorted by (row, point index).  One count launch, one read-back, one fill launch."""
    L.require_device(points, boxes, scores, transforms, deco_boxes)
    n, N, cap = _check_rows(points, boxes, scores, transforms, attr_dims, point_cloud_range, max_points, deco_boxes)
    return _rows(points, boxes, scores, n, N, cap, None, transforms, extra_width, attr_dims, point_cloud_range, deco_boxes)


def frame_major(frame_rows, frames):
    """The host's plan of a frames call: ``order``, the caller's rows sorted by frame (stable: a frame's rows keep the
    caller's order), and box_offsets [frames + 1], where each frame's rows lie in that order -- Python ints."""
    order = sorted(range(len(frame_rows)), key=frame_rows.__getitem__)
    offsets = [0] * (frames + 1)
    for f in frame_rows:
        offsets[f + 1] += 1
    for f in range(frames):
        offsets[f + 1] += offsets[f]
    return order, offsets


def scene_steps_rows(points, cloud_sizes, boxes, scores, frame_rows, transforms=None, extra_width=EXTRA_WIDTH, attr_dims=2,
                     point_cloud_range=None, max_points=-1, deco_boxes=None):
    """scene_step_rows for the clouds of F sensor frames in one call (TrackletRoIHeadOCC.simple_test_scene_steps): ``points``
    [N, >= 3 + attr_dims] f32, the F clouds concatenated, ``cloud_sizes`` their F lengths (ints on the host); boxes [n, 7],
    scores [n], transforms [n, 12] and deco_boxes [n, 7] per ROW in the caller's order, as in scene_step_rows;
    ``frame_rows`` n ints on the host: the cloud 0..F-1 a row belongs to -- its box lies in that cloud's frame and takes
    that cloud's points only.  The rows need not be grouped by frame (a chunked step has them slot-major).

    Returns what scene_step_rows returns, as if it had been called once per frame and the results put in the caller's row
    order, bit for bit: (xyz [M, 3], feats [M, attr_dims + 5], row [M] i64 = the CALLER's row, counts [n] i64 on the host,
    uncapped, in the caller's order), sorted by (row, point index within the frame).

    The frame-major order of the boxes is made on the host (frame_major); the whole call is one upload of offsets and
    order, one count launch, one read-back, one upload of totals and first output rows, one fill launch that writes every
    row at its final place (ococc_scene_rows_frames_count / _fill, csrc/scene_rows.hip).

    Reported before any launch (OcoccError): what scene_step_rows reports, cloud_sizes that hold a negative or do not sum
    to N, more than 65535 clouds, frame_rows of another length than n or outside 0..F-1."""
    n, N, cap = _check_rows(points, boxes, scores, transforms, attr_dims, point_cloud_range, max_points, deco_boxes)
    sizes, frame_rows = [int(v) for v in cloud_sizes], [int(v) for v in frame_rows]
    F = len(sizes)
    if any(v < 0 for v in sizes) or sum(sizes) != N:
        raise L.OcoccError(f'cloud_sizes {sizes[:8]}{"..." if F > 8 else ""} must be >= 0 and sum to the {N} points given')
    if F > 65535:
        raise L.OcoccError(f'{F} clouds in one call: at most 65535')
    if len(frame_rows) != n or any(not 0 <= f < F for f in frame_rows):
        raise L.OcoccError(f'frame_rows must hold the cloud 0..{F - 1} of each of the {n} rows, got {len(frame_rows)} values'
                           + (f' from {min(frame_rows)} to {max(frame_rows)}' if frame_rows else ''))
    L.require_device(points, boxes, scores, transforms, deco_boxes)
    return _rows(points, boxes, scores, n, N, cap, (sizes, frame_rows), transforms, extra_width, attr_dims,
                 point_cloud_range, deco_boxes)


def _rows(points, boxes, scores, n, N, cap, frames, transforms, extra_width, attr_dims, point_cloud_range, deco_boxes):
    """the body of scene_step_rows (``frames`` None: the one-cloud exports, whose fill pass reads the prefix tables
    [n + 1] of the counts and of the kept) and scene_steps_rows (``frames`` = (cloud_sizes, frame_rows): the plan, the
    many-cloud exports, whose fill pass reads every box's total and first output row) over checked arguments"""
    dev = points.device
    points, crop, row_feats, transforms, rng = _row_inputs(points, boxes, scores, transforms, extra_width, point_cloud_range,
                                                           deco_boxes)
    A, K = int(attr_dims), row_feats.size(1)
    counts = torch.zeros((n,), dtype=torch.int64)
    empty = lambda: (torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, A + K), dtype=torch.float32, device=dev),
                     torch.zeros((0,), dtype=torch.int64, device=dev), counts)
    if n == 0 or N == 0:
        return empty()
    # one cloud: the boxes stay in the caller's order and the exports take no plan
    what, order, max_pts, caller_rows = 'scene_rows', slice(None), N, ()
    head = (L.ptr(points), N, points.size(1), L.ptr(crop), n, L.ptr(transforms), rng)
    if frames is not None:
        (sizes, frame_rows), what = frames, 'scene_rows_frames'
        F = len(sizes)
        order, box_offsets = frame_major(frame_rows, F)
        cloud_offsets = [0] * (F + 1)
        for f, v in enumerate(sizes):
            cloud_offsets[f + 1] = cloud_offsets[f] + v
        max_pts, max_boxes = max(sizes), max(box_offsets[f + 1] - box_offsets[f] for f in range(F))
        plan = torch.from_numpy(np.array(cloud_offsets + box_offsets + order, dtype=np.int64)).to(dev)   # (one upload)
        cloud_off, box_off, order_dev = plan[:F + 1], plan[F + 1:2 * F + 2], plan[2 * F + 2:]
        if order != list(range(n)):                              # the boxes and what goes with them, grouped by frame
            crop, row_feats = crop[order_dev], row_feats[order_dev]
            transforms = None if transforms is None else transforms[order_dev]
        caller_rows = (L.ptr(order_dev),)
        head = (L.ptr(points), N, points.size(1), L.ptr(cloud_off), L.ptr(crop), n, L.ptr(box_off), F, max_pts, max_boxes,
                L.ptr(transforms), rng)
    counts_dev = torch.zeros((n,), dtype=torch.int64, device=dev)
    ws_bytes = int(L.lib.ococc_scene_rows_workspace_bytes(max_pts, n))
    ws = L.workspace(ws_bytes, dev)
    L.check(getattr(L.lib, f'ococc_{what}_count')(*head, L.ptr(counts_dev), L.ptr(ws), ws_bytes, L.stream()), f'{what}_count')
    totals = counts_dev.cpu().numpy()                            # the read-back (frames: frame-major)
    per_row = counts.numpy()                                     # (the same memory: numpy for the host's few integers)
    per_row[order] = totals                                      # the caller's order
    kept = np.minimum(per_row, cap) if cap > 0 else per_row
    ends = np.cumsum(kept)
    M = int(ends[-1])
    if M == 0:
        return empty()
    # what the fill pass reads per box -- one cloud: the prefix tables [n + 1] of the counts and of the kept; frames: the
    # total and the first output row of every box, frame-major
    if frames is None:
        scans = np.zeros((2, n + 1), dtype=np.int64)
        np.cumsum(totals, out=scans[0, 1:])
        scans[1, 1:] = ends
    else:
        scans = np.stack([totals, (ends - kept)[order]])
    scans_dev = torch.from_numpy(scans).to(dev)                  # (one upload for both)
    xyz = L.empty((M, 3), torch.float32, dev)
    feats = L.empty((M, A + K), torch.float32, dev)
    row = L.empty((M,), torch.int64, dev)
    L.check(getattr(L.lib, f'ococc_{what}_fill')(
        *head, A, L.ptr(row_feats), K, *caller_rows, cap, L.ptr(scans_dev[0]), L.ptr(scans_dev[1]),
        *(() if frames is None else (M,)), L.ptr(xyz), L.ptr(feats), L.ptr(row), L.ptr(ws), ws_bytes, L.stream()), f'{what}_fill')
    return xyz, feats, row, counts
