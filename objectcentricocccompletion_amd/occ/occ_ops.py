"""Host mirror of mmdet3d/ops/occ/occ_ops.py: voxel-centre helpers of the implicit
occupancy grid (generate_dense_voxel_centers :5-50, quantize_points :53-93,
jitter_voxel_center :96-100).  Elementwise index math on small tensors."""
import os

import torch

from .._lib import const_tensor


def generate_dense_voxel_centers(bbox_sizes, voxel_size, scale_wlh=[1.0, 1.0, 1.0],
                                 offset_wlh=[0.0, 0.0, 0.0], as_volume=False):
    """Centres of the ceil(size / voxel) cells of each box, in the box frame (origin at the
    box centre), x fastest last: list of [X*Y*Z, 3] (or [X,Y,Z,3]) tensors."""
    out = []
    for size in bbox_sizes:
        size = size * size.new_tensor(scale_wlh) + size.new_tensor(offset_wlh)
        n = torch.ceil(size / voxel_size)
        xs, ys, zs = [int(v) for v in n.tolist()]
        dev = bbox_sizes.device
        gx, gy, gz = torch.meshgrid(torch.arange(xs, device=dev), torch.arange(ys, device=dev),
                                    torch.arange(zs, device=dev), indexing='ij')
        coors = torch.stack([gx, gy, gz], dim=-1).view(-1, 3)
        centers = coors.to(torch.float) * voxel_size + (-size / 2) + voxel_size / 2
        if as_volume:
            centers = centers.view(xs, ys, zs, 3)
        out.append(centers)
    return out


def quantize_points(points, rois, rois_points_idx, voxel_size, scale_wlh=[1.0, 1.0, 1.0],
                    offset_wlh=[0.0, 0.0, 0.0], to_center=False):
    """Voxel index floor((p + size/2) / voxel) of box-frame points, the volume centred on the
    (enlarged) RoI of each point; with to_center the centre of that voxel (occ_ops.py:53-93)."""
    sizes = rois[:, 4:7]
    sizes = sizes * const_tensor(scale_wlh, sizes.device, sizes.dtype).view(1, 3) \
        + const_tensor(offset_wlh, sizes.device, sizes.dtype).view(1, 3)
    min_bound = (-sizes / 2)[rois_points_idx.long()]
    voxel_coors = torch.floor((points - min_bound) / voxel_size).to(torch.long)
    if to_center:
        return voxel_coors.to(torch.float) * voxel_size + min_bound + voxel_size / 2
    return voxel_coors


def jitter_voxel_center(voxel_size, voxel_centers):
    return voxel_centers + torch.rand_like(voxel_centers) * voxel_size - voxel_size / 2


def dense_voxel_centers_batched(bbox_sizes, voxel_size, scale_wlh=[1.0, 1.0, 1.0], offset_wlh=[0.0, 0.0, 0.0]):
    """All boxes of generate_dense_voxel_centers in one flat tensor: (centers [sum K, 3], box index [sum K],
    K per box [R]).  Same cell order (x slowest, z fastest) and the same float expression per element, so
    ``centers[box == j]`` equals ``generate_dense_voxel_centers(...)[j]`` bit for bit; one host read-back
    (the total) instead of a Python loop over boxes."""
    dev = bbox_sizes.device
    if bbox_sizes.size(0) == 0:
        z = torch.zeros((0,), dtype=torch.long, device=dev)
        return bbox_sizes.new_zeros((0, 3)), z, z
    size = bbox_sizes * bbox_sizes.new_tensor(scale_wlh) + bbox_sizes.new_tensor(offset_wlh)     # [R,3]
    dims = torch.ceil(size / voxel_size).to(torch.long)                                             # [R,3]
    k = dims[:, 0] * dims[:, 1] * dims[:, 2]
    total = int(k.sum())
    start = torch.cumsum(k, 0) - k
    box = torch.repeat_interleave(torch.arange(size.size(0), device=dev), k, output_size=total)
    local = torch.arange(total, device=dev) - start[box]
    ys, zs = dims[box, 1], dims[box, 2]
    coors = torch.stack([local // (ys * zs), (local // zs) % ys, local % zs], 1)
    centers = coors.to(torch.float) * voxel_size + (-size / 2)[box] + voxel_size / 2
    return centers, box, k


def occ_iou_count(logits, labels, counts, row0, pos_thresh, roi_xyz=None, half_sizes=None):
    """Adds the occupancy (inter, union) of n RoIs to rows [row0, row0 + n) of ``counts`` (int64 [R, 2], on the device)
    in one launch (csrc/occ_iou_count.hip): logits [n*K] or [n, K] f32 of the one-logit decoder, labels [K] int64
    (occupied: == 1); with roi_xyz [n, K, 3] and half_sizes [n, 3] a cell outside its RoI's box counts as predicted
    empty.  Predicted occupied is sigmoid(logit) > pos_thresh, decided as ATen decides it.  Nothing is read back."""
    from .. import _lib as L
    L.require_device(logits, labels, counts, roi_xyz, half_sizes)
    K = labels.numel()
    n = logits.numel() // K if K else 0
    if logits.dtype != torch.float32 or logits.numel() != n * K:
        raise L.OcoccError(f'occ_iou_count: logits {tuple(logits.shape)} {logits.dtype} are not f32 [n, {K}]')
    if labels.dtype != torch.int64 or counts.dtype != torch.int64 or counts.dim() != 2 or counts.size(1) != 2 \
            or not counts.is_contiguous():
        raise L.OcoccError('occ_iou_count: labels and counts are int64, counts a contiguous [R, 2] buffer')
    if (roi_xyz is None) != (half_sizes is None):
        raise L.OcoccError('occ_iou_count: roi_xyz and half_sizes go together')
    if roi_xyz is not None:
        if roi_xyz.dtype != torch.float32 or roi_xyz.numel() != n * K * 3 or half_sizes.dtype != torch.float32 \
                or half_sizes.numel() != n * 3:
            raise L.OcoccError(f'occ_iou_count: roi_xyz / half_sizes are not f32 [{n}, {K}, 3] / [{n}, 3]')
        roi_xyz, half_sizes = roi_xyz.contiguous(), half_sizes.contiguous()
    logits, labels = logits.contiguous(), labels.contiguous()
    L.check(L.lib.ococc_occ_iou_count(L.ptr(logits), L.ptr(labels), L.ptr(roi_xyz), L.ptr(half_sizes), n, K,
                                      float(pos_thresh), L.ptr(counts), int(row0), counts.size(0), L.stream()),
            'occ_iou_count')
    return counts


def _loss_mask_shapes(L, what, xyz, box_size, score, labels, ori_logits, outside, observed, unmatched):
    """(M, K) of the sample masks' inputs, or OcoccError: score [M] f32, labels [M * K] int64, and -- where a switch reads
    them -- xyz [M * K, 3] f32, box_size [M, 3] f32, ori_logits [M * K] f32."""
    if score is None or labels is None or score.dtype != torch.float32 or labels.dtype != torch.int64:
        raise L.OcoccError(f'{what}: score is f32 [M] and labels int64 [M * K]')
    M, N = score.numel(), labels.numel()
    if (N % M if M else N) != 0:
        raise L.OcoccError(f'{what}: {N} labels for {M} RoIs')
    K = N // M if M else 0
    if outside and (xyz is None or box_size is None or xyz.dtype != torch.float32 or box_size.dtype != torch.float32
                    or xyz.numel() != N * 3 or box_size.numel() != M * 3 or xyz.size(-1) != 3 or box_size.size(-1) != 3):
        raise L.OcoccError(f'{what}: no_loss_for_outside needs xyz f32 [{M} * {K}, 3] and box_size f32 [{M}, 3]')
    if (observed or unmatched) and (ori_logits is None or ori_logits.dtype != torch.float32 or ori_logits.numel() != N):
        raise L.OcoccError(f'{what}: the observed / unmatched masks need ori_logits f32 [{M} * {K}] of the one-logit decoder')
    return M, K


def occ_loss_masks(score, score_thresh, labels, xyz=None, box_size=None, ori_logits=None, pos_thresh=0.5, outside=False,
                   observed=False, unmatched=False):
    """The sample weights of OccBBoxHead.loss_occ under its train_cfg switches in one launch (csrc/occ_loss_masks.hip),
    sample k of positive RoI i in row i * K + k:
        weights [M * K] f32 = (score[i] > score_thresh)                                   (ococc_bbox_head.py:708-710)
            * (-box_size[i] / 2 <= xyz <= box_size[i] / 2 on all axes)  with ``outside``   (:713-722; NaN is outside)
            * (class of ori_logits == 0)                                  with ``observed``  (:723-734)
        unmatched [M * K] uint8 = (labels == 1) != (class of ori_logits), with ``unmatched`` (:749-752), else None
        counts [3] int64 on the device: #(weights > 0), #unmatched, #(unmatched and weights > 0)
    class = sigmoid(logit) > pos_thresh, decided as ATen decides it (NaN: class 0).  Nothing is read back; two calls give
    the same bits.  ``occ_loss_masks_aten`` is the same result as a torch operator chain."""
    from .. import _lib as L
    L.require_device(score, labels, xyz, box_size, ori_logits)
    M, K = _loss_mask_shapes(L, 'occ_loss_masks', xyz, box_size, score, labels, ori_logits, outside, observed, unmatched)
    dev = score.device
    flags = (1 if outside else 0) | (2 if observed else 0) | (4 if unmatched else 0)
    weights = L.empty((M * K,), torch.float32, dev)
    um = L.empty((M * K,), torch.uint8, dev) if unmatched else None
    counts = L.empty((3,), torch.int64, dev)
    c = lambda t, on: t.contiguous() if (on and t is not None) else None
    xyz, box_size = c(xyz, outside), c(box_size, outside)
    ori_logits, lab = c(ori_logits, observed or unmatched), c(labels, unmatched)
    L.check(L.lib.ococc_occ_loss_masks_f32(L.ptr(xyz), L.ptr(box_size), L.ptr(score.contiguous()), L.ptr(ori_logits), L.ptr(lab),
                                           M, K, float(score_thresh), float(pos_thresh), flags, L.ptr(weights), L.ptr(um),
                                           L.ptr(counts), L.stream()), 'occ_loss_masks')
    return weights, um, counts


def occ_loss_masks_aten(score, score_thresh, labels, xyz=None, box_size=None, ori_logits=None, pos_thresh=0.5,
                        outside=False, observed=False, unmatched=False):
    """``occ_loss_masks`` as the reference's operator chain (ococc_bbox_head.py:706-710, 713-722, 730-734, 749-753, 792),
    on any device: what OccBBoxHead.loss_occ takes on CPU tensors or with OCOCC_OCC_LOSS_KERNEL=0, and the yardstick of the
    kernel."""
    from .. import _lib as L
    M, K = _loss_mask_shapes(L, 'occ_loss_masks_aten', xyz, box_size, score, labels, ori_logits, outside, observed, unmatched)
    score = score.reshape(-1)
    occ_weights = torch.zeros_like(score)
    occ_weights[score > score_thresh] = 1
    occ_weights = occ_weights.view(M, 1).repeat(1, K)
    if outside:
        xyz, size = xyz.reshape(M, K, 3), box_size.reshape(M, 3)
        inside = (xyz >= -size[:, None, :] / 2).all(dim=-1) & (xyz <= size[:, None, :] / 2).all(dim=-1)
        occ_weights = occ_weights * inside.float()
    if observed or unmatched:
        ori_cls = (ori_logits.reshape(M, K).sigmoid() > pos_thresh).long()     # get_cls_from_pred, cls_dim 1
    if observed:
        occ_weights = occ_weights * (ori_cls == 0).float()
    weights = occ_weights.view(-1)
    valid = weights > 0
    um = None
    zero = valid.sum() * 0
    if unmatched:
        um = (labels.reshape(-1) == 1).long() != ori_cls.view(-1)
    counts = torch.stack([valid.sum(), um.sum() if unmatched else zero, (um & valid).sum() if unmatched else zero])
    return weights, um.to(torch.uint8) if unmatched else None, counts


def dense_grid_layout(bbox_sizes, voxel_size, scale_wlh=[1.0, 1.0, 1.0], offset_wlh=[0.0, 0.0, 0.0]):
    """The grid of every box as the kernels of csrc/occ_export.hip take it: (enlarged sizes [R, 3] f32, dims [R, 3] i32,
    start [R + 1] i64 the exclusive prefix of the cells per box, total).  Built on the device with the expressions of
    dense_voxel_centers_batched; the total is the one read-back."""
    size = (bbox_sizes * bbox_sizes.new_tensor(scale_wlh) + bbox_sizes.new_tensor(offset_wlh)).contiguous()
    dims = torch.ceil(size / voxel_size).to(torch.long)
    start = torch.zeros(size.size(0) + 1, dtype=torch.long, device=size.device)
    if size.size(0):
        torch.cumsum(dims[:, 0] * dims[:, 1] * dims[:, 2], 0, out=start[1:])
    return size, dims.to(torch.int32), start, int(start[-1]) if size.size(0) else 0


def _check_layout(L, what, sizes, dims, start):
    R = sizes.size(0) if sizes.dim() == 2 else -1
    if sizes.dtype != torch.float32 or sizes.dim() != 2 or sizes.size(1) != 3 or dims.dtype != torch.int32 \
            or tuple(dims.shape) != (R, 3) or start.dtype != torch.int64 or tuple(start.shape) != (R + 1,):
        raise L.OcoccError(f'{what}: sizes f32 [R, 3], dims int32 [R, 3] and start int64 [R + 1] expected, got '
                           f'{tuple(sizes.shape)} {sizes.dtype}, {tuple(dims.shape)} {dims.dtype}, '
                           f'{tuple(start.shape)} {start.dtype}')
    return R


def dense_grid_cells(sizes, dims, start, voxel_size, lo, hi, total):
    """Cells [lo, hi) of the flat cell list of dense_grid_layout in one launch (csrc/occ_export.hip): (centres
    [hi - lo, 3] f32 in the box frame, box index [hi - lo] int32), bit for bit rows lo..hi of
    dense_voxel_centers_batched.  ``total``: the number of cells dense_grid_layout returned (hi beyond it is refused).
    Nothing is read back."""
    from .. import _lib as L
    L.require_device(sizes, dims, start)
    R = _check_layout(L, 'dense_grid_cells', sizes, dims, start)
    lo, hi = int(lo), int(hi)
    if hi < lo or lo < 0 or hi > int(total):
        raise L.OcoccError(f'dense_grid_cells: cell range [{lo}, {hi}) of {int(total)} cells')
    centers = L.empty((hi - lo, 3), torch.float32, sizes.device)
    index = L.empty((hi - lo,), torch.int32, sizes.device)
    L.check(L.lib.ococc_dense_grid_cells_f32(L.ptr(sizes.contiguous()), L.ptr(dims.contiguous()), L.ptr(start.contiguous()),
                                             R, float(voxel_size), lo, hi, L.ptr(centers), L.ptr(index), L.stream()),
            'dense_grid_cells')
    return centers, index


def occ_select(logits, sizes, dims, start, total, voxel_size, pos_thresh, rois=None, roi_values=None, with_score=False):
    """The occupied cells (sigmoid(logit) > pos_thresh, as ATen decides it) of the flat cell list, in cell order:
    (points [n_occ, 3 or 4] f32 on the device, counts per box as a list of int).  logits [N] or [N, 1] f32 of the
    one-logit decoder, N == ``total``, the number of cells dense_grid_layout returned.  Columns 0-2: the cell centre in the box frame, or with ``rois`` ([R, >= 8]: batch, x, y, z, w, l,
    h, yaw) in the LiDAR frame by OccDecoder._to_lidar's arithmetic; column 3: ``roi_values[box]`` when given, else (with
    ``with_score``) sigmoid(logit).  One count launch, one scan, one fill launch (csrc/occ_export.hip); the one
    read-back is the per-box counts."""
    from .. import _lib as L
    L.require_device(logits, sizes, dims, start, rois, roi_values)
    R = _check_layout(L, 'occ_select', sizes, dims, start)
    n = logits.numel()
    if logits.dtype != torch.float32 or (logits.dim() == 2 and logits.size(1) != 1) or logits.dim() > 2:
        raise L.OcoccError(f'occ_select: logits {tuple(logits.shape)} {logits.dtype} are not f32 [N] or [N, 1]')
    if n != int(total):
        raise L.OcoccError(f'occ_select: {n} logits for a layout of {int(total)} cells')
    if rois is not None and (rois.dtype != torch.float32 or rois.dim() != 2 or rois.size(0) != R or rois.size(1) < 8):
        raise L.OcoccError(f'occ_select: rois {tuple(rois.shape)} {rois.dtype} are not f32 [{R}, >= 8]')
    if roi_values is not None and (roi_values.dtype != torch.float32 or roi_values.numel() != R):
        raise L.OcoccError(f'occ_select: roi_values {tuple(roi_values.shape)} {roi_values.dtype} are not f32 [{R}]')
    dev = logits.device
    cols = 4 if (roi_values is not None or with_score) else 3
    if R == 0:
        return L.empty((0, cols), torch.float32, dev), []
    logits, sizes, dims, start = logits.contiguous(), sizes.contiguous(), dims.contiguous(), start.contiguous()
    tiles = int(L.lib.ococc_occ_select_max_tiles(n, R))
    tile_start = L.empty((R + 1,), torch.int64, dev)
    pose = rois.contiguous() if rois is not None else None
    value = roi_values.contiguous().view(-1) if roi_values is not None else None

    def count(tile_counts, roi_counts):
        L.check(L.lib.ococc_occ_select_count(L.ptr(logits), n, L.ptr(start), R, float(pos_thresh), L.ptr(tile_start),
                                             L.ptr(tile_counts), tiles, L.ptr(roi_counts), L.stream()), 'occ_select_count')

    def fill(scan, out, n_occ):
        cos, sin = (f(pose[:, 7]).contiguous() if pose is not None else None for f in (torch.cos, torch.sin))
        L.check(L.lib.ococc_occ_select_fill(L.ptr(logits), n, L.ptr(start), L.ptr(tile_start), R, float(pos_thresh),
                                            L.ptr(scan), tiles, L.ptr(sizes), L.ptr(dims), float(voxel_size),
                                            int(pose is not None), L.ptr(pose), pose.size(1) if pose is not None else 0,
                                            L.ptr(cos), L.ptr(sin), L.ptr(value), cols, L.ptr(out), n_occ, L.stream()),
                'occ_select_fill')

    return L.count_scan_fill(tiles, R, cols, dev, count, fill)[:2]


# ---------------------------------------------------------------------------------------------------------------------
# completed occupancy of one online step (csrc/occ_frame.hip)
def _frame_select_shapes(L, what, logits, sizes, dims, start, total, rois, local_xyz, pts_roi, row_keep, transforms,
                         two_logits):
    """(R, M) of the inputs of occ_frame_select / occ_frame_select_aten, or OcoccError."""
    R = _check_layout(L, what, sizes, dims, start)
    wide = (1, 2) if two_logits else (1,)
    if logits.dtype != torch.float32 or logits.dim() > 2 or (logits.dim() == 2 and logits.size(1) not in wide):
        raise L.OcoccError(f'{what}: logits {tuple(logits.shape)} {logits.dtype} are not f32 [N] or [N, 1]'
                           + (' (or [N, 2] of the two-logit decoder)' if two_logits else ''))
    n = logits.size(0) if logits.dim() == 2 else logits.numel()
    if n != int(total):
        raise L.OcoccError(f'{what}: {n} logits for a layout of {int(total)} cells')
    if rois is None or rois.dtype != torch.float32 or rois.dim() != 2 or rois.size(0) != R or rois.size(1) < 8:
        raise L.OcoccError(f'{what}: rois are f32 [{R}, >= 8] (batch, x, y, z, w, l, h, yaw): the pose of every grid')
    if local_xyz is None or pts_roi is None or local_xyz.dtype != torch.float32 or local_xyz.dim() != 2 \
            or local_xyz.size(1) != 3 or pts_roi.dtype not in (torch.int32, torch.int64) \
            or tuple(pts_roi.shape) != (local_xyz.size(0),):
        raise L.OcoccError(f'{what}: local_xyz is f32 [M, 3] and pts_roi int32 (or int64) [M]')
    if row_keep is not None and (row_keep.dtype not in (torch.uint8, torch.bool) or tuple(row_keep.shape) != (R,)):
        raise L.OcoccError(f'{what}: row_keep is uint8 (or bool) [{R}]')
    if transforms is not None and (transforms.dtype != torch.float32 or transforms.numel() != R * 12
                                   or transforms.size(0) != R):
        raise L.OcoccError(f'{what}: transforms are f32 [{R}, 12] (or [{R}, 3, 4]), row-major 3x4')
    return R, local_xyz.size(0)


def occ_frame_select(logits, sizes, dims, start, total, voxel_size, pos_thresh, rois, local_xyz, pts_roi,
                     scale_wlh=[1.0, 1.0, 1.0], offset_wlh=[0.0, 0.0, 0.0], row_keep=None, transforms=None, observed=True):
    """The completed occupancy of one step from the flat cell list of dense_grid_layout (``sizes`` are its enlarged
    sizes: rois[:, 4:7] * scale_wlh + offset_wlh): every cell that is predicted occupied (sigmoid(logit) > pos_thresh,
    as ATen decides it) or -- with ``observed`` -- holds one of the pooled points ``local_xyz`` [M, 3] (box frame, the
    coordinates OccAutoEncoder.sample_observation quantises; ``pts_roi`` [M] their RoI), of every RoI whose ``row_keep``
    byte is non-zero (None: all).  Returns (out [N, 4] f32: x, y, z in the LiDAR frame of ``rois`` [R, >= 8] -- through
    ``transforms`` [R, 12], row-major 3x4, when given -- and sigmoid(logit); flags [N] uint8, bit 0 predicted, bit 1
    observed; counts per RoI as a list of int), rows in cell order, RoI after RoI.  One memset and one mark launch, one
    count launch, one scan, one fill launch (csrc/occ_frame.hip); the one read-back is the per-RoI counts.
    ``occ_frame_select_aten`` is the same result as a torch operator chain."""
    from .. import _lib as L
    R, M = _frame_select_shapes(L, 'occ_frame_select', logits, sizes, dims, start, total, rois, local_xyz, pts_roi,
                                row_keep, transforms, two_logits=False)
    L.require_device(logits, sizes, dims, start, rois, local_xyz, pts_roi, row_keep, transforms)
    dev = logits.device
    n = int(total)
    if R == 0:
        return L.empty((0, 4), torch.float32, dev), L.empty((0,), torch.uint8, dev), []
    logits, sizes, dims, start = logits.contiguous(), sizes.contiguous(), dims.contiguous(), start.contiguous()
    rois = rois.contiguous()
    seen = None
    if observed:
        seen = L.empty((n,), torch.uint8, dev)
        L.check(L.lib.ococc_occ_frame_mark(L.ptr(local_xyz.contiguous()), L.ptr(pts_roi.to(torch.int32).contiguous()), M,
                                           L.ptr(sizes), L.ptr(dims), L.ptr(start), R, float(voxel_size), L.ptr(seen), n,
                                           L.stream()), 'occ_frame_mark')
    if row_keep is not None:
        row_keep = row_keep.contiguous().view(torch.uint8) if row_keep.dtype == torch.bool else row_keep.contiguous()
    tiles = int(L.lib.ococc_occ_select_max_tiles(n, R))
    tile_start = L.empty((R + 1,), torch.int64, dev)
    cos, sin = torch.cos(rois[:, 7]).contiguous(), torch.sin(rois[:, 7]).contiguous()
    transforms = transforms.contiguous() if transforms is not None else None

    def count(tile_counts, roi_counts):
        L.check(L.lib.ococc_occ_frame_count(L.ptr(logits), L.ptr(seen), L.ptr(row_keep), n, L.ptr(start), R,
                                            float(pos_thresh), L.ptr(tile_start), L.ptr(tile_counts), tiles,
                                            L.ptr(roi_counts), L.stream()), 'occ_frame_count')

    def fill(scan, out, n_out):
        flags = L.empty((n_out,), torch.uint8, dev)
        L.check(L.lib.ococc_occ_frame_fill(L.ptr(logits), L.ptr(seen), L.ptr(row_keep), n, L.ptr(start), L.ptr(tile_start),
                                           R, float(pos_thresh), L.ptr(scan), tiles, L.ptr(sizes), L.ptr(dims),
                                           float(voxel_size), L.ptr(rois), rois.size(1), L.ptr(cos), L.ptr(sin),
                                           L.ptr(transforms), L.ptr(out), L.ptr(flags), n_out, L.stream()), 'occ_frame_fill')
        return flags

    out, counts, flags = L.count_scan_fill(tiles, R, 4, dev, count, fill)
    return out, flags, counts


def _observed_aten(size, dims, start, total, voxel_size, local_xyz, pts_roi):
    """observed [total] bool of the flat cell list, the mark kernel of csrc/occ_frame.hip as an operator chain: ``size``
    [R, 3] the enlarged sizes, ``local_xyz`` [M, 3] the pooled points in the box frame, ``pts_roi`` [M] their RoI."""
    dev = local_xyz.device
    seen = torch.zeros(int(total), dtype=torch.bool, device=dev)
    idx = pts_roi.long()
    # quantize_points' expression with the voxel as a TENSOR divisor: on a device ATen divides by a host scalar through
    # its reciprocal, which moves a point that sits on a cell face (2.0 / 0.2f is 10, 2.0 * (1 / 0.2f) is 9.9999998);
    # tensor / tensor is a true division everywhere, as on the host and in the mark kernel
    coors = torch.floor((local_xyz - (-size / 2)[idx]) / const_tensor((voxel_size,), dev)).to(torch.long)
    d = dims.long()[idx]
    valid = ((coors < d) & (coors >= 0)).all(dim=1)
    flat = start[idx] + (coors[:, 0] * d[:, 1] + coors[:, 1]) * d[:, 2] + coors[:, 2]
    seen[flat[valid]] = True
    return seen


def occ_frame_select_aten(logits, sizes, dims, start, total, voxel_size, pos_thresh, rois, local_xyz, pts_roi,
                          scale_wlh=[1.0, 1.0, 1.0], offset_wlh=[0.0, 0.0, 0.0], row_keep=None, transforms=None,
                          observed=True):
    """``occ_frame_select`` as an operator chain on any device: the rasterisation of OccAutoEncoder.sample_observation
    (quantize_points' expression with a true division on every device, flat cell ids, one scatter), OccDecoder._occupied,
    a boolean index, OccDecoder._to_lidar and a batched matrix product.  What CPU tensors, two-logit decoders (logits [N, 2]) and OCOCC_OCC_FRAME_KERNEL=0 take, and
    what the kernels are timed against.  ``sizes``, ``dims`` and ``start`` are checked and ``start`` is used; the cell
    centres come from dense_voxel_centers_batched of the same rois, scale_wlh and offset_wlh."""
    from .. import _lib as L
    from .occ_base import OccDecoder
    R, M = _frame_select_shapes(L, 'occ_frame_select_aten', logits, sizes, dims, start, total, rois, local_xyz, pts_roi,
                                row_keep, transforms, two_logits=True)
    dev = logits.device
    if R == 0:
        return logits.new_zeros((0, 4)), torch.zeros((0,), dtype=torch.uint8, device=dev), []
    centers, box, _ = dense_voxel_centers_batched(rois[:, 4:7], voxel_size, scale_wlh, offset_wlh)
    if logits.dim() == 2 and logits.size(1) == 2:
        pred, prob = logits[:, 1] > logits[:, 0], logits.softmax(-1)[:, 1]
    else:
        prob = logits.sigmoid().view(-1)
        pred = prob > pos_thresh
    seen = torch.zeros(int(total), dtype=torch.bool, device=dev)
    if observed and M:
        size = rois[:, 4:7] * const_tensor(scale_wlh, dev).view(1, 3) + const_tensor(offset_wlh, dev).view(1, 3)
        seen = _observed_aten(size, dims, start, total, voxel_size, local_xyz, pts_roi)
    sel = pred | seen
    if row_keep is not None:
        sel = sel & (row_keep != 0)[box]
    pbox = box[sel]
    pts = OccDecoder._to_lidar(centers[sel], pbox, rois[:, 1:4], rois[:, 4:7], rois[:, 7])
    if transforms is not None:
        m = transforms.reshape(R, 3, 4)[pbox]
        pts = torch.bmm(m[:, :, :3], pts[:, :, None]).squeeze(2) + m[:, :, 3]
    out = torch.cat([pts, prob[sel].view(-1, 1)], 1)
    flags = pred[sel].to(torch.uint8) | (seen[sel].to(torch.uint8) << 1)
    return out, flags, torch.bincount(pbox, minlength=R).tolist()


# ---------------------------------------------------------------------------------------------------------------------
# observation sample of a tuned online step (csrc/tune_sample.hip)
# 0: tune_sample runs the operator chain tune_sample_aten instead of the kernels
TUNE_SAMPLE_KERNEL = os.environ.get('OCOCC_TUNE_SAMPLE_KERNEL', '1') != '0'

_M64 = (1 << 64) - 1
TUNE_GOLDEN, TUNE_CAP_SALT = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03   # csrc/tune_rng.hpp


def _i64(v):
    """the 64-bit pattern ``v`` as the Python int an int64 tensor holds"""
    v &= _M64
    return v - (1 << 64) if v >= (1 << 63) else v


def mix64_int(x):
    """The splitmix64 finaliser of one Python int (csrc/tune_rng.hpp), as an unsigned 64-bit value."""
    x &= _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def tune_row_seed(seed, slot, frame):
    """The seed of the sample of frame ``frame`` of cache slot ``slot``: mix64(seed ^ (slot << 32 | frame)) as the signed
    value an int64 tensor holds.  A function of (seed, slot, frame) alone: the draw does not depend on the row's place in
    the call."""
    return _i64(mix64_int((int(seed) & _M64) ^ (((int(slot) << 32) | int(frame)) & _M64)))


def _lsr(x, n):
    """logical right shift of an int64 tensor"""
    return (x >> n) & ((1 << (64 - n)) - 1)


def _tune_key(seed, c):
    """key(seed, c) of csrc/tune_rng.hpp on int64 tensors (two's-complement products wrap as the u64 ones do): values
    in [0, 2^32)."""
    x = seed + (c + 1) * _i64(TUNE_GOLDEN)
    x = (x ^ _lsr(x, 30)) * _i64(0xBF58476D1CE4E5B9)
    x = (x ^ _lsr(x, 27)) * _i64(0x94D049BB133111EB)
    return _lsr(x ^ _lsr(x, 31), 32)


def _rank_in_group(group, key, group_start):
    """rank of every element among the elements of its group by (key, position); ``group`` ascending, key < 2^32"""
    order = torch.argsort((group << 32) | key, stable=True)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel(), device=order.device)
    return rank - group_start[group]


def _tune_sample_shapes(L, what, sizes, dims, start, total, local_xyz, pts_roi, row_seeds, row_keep, balance, cap):
    """(K, M) of the inputs of tune_sample / tune_sample_aten, or OcoccError."""
    K = _check_layout(L, what, sizes, dims, start)
    if local_xyz is None or pts_roi is None or local_xyz.dtype != torch.float32 or local_xyz.dim() != 2 \
            or local_xyz.size(1) != 3 or pts_roi.dtype not in (torch.int32, torch.int64) \
            or tuple(pts_roi.shape) != (local_xyz.size(0),):
        raise L.OcoccError(f'{what}: local_xyz is f32 [M, 3] and pts_roi int32 (or int64) [M]')
    if row_seeds is None or row_seeds.dtype != torch.int64 or tuple(row_seeds.shape) != (K,):
        raise L.OcoccError(f'{what}: row_seeds is int64 [{K}]')
    if row_keep is not None and (row_keep.dtype not in (torch.uint8, torch.bool) or tuple(row_keep.shape) != (K,)):
        raise L.OcoccError(f'{what}: row_keep is uint8 (or bool) [{K}]')
    if int(total) < 0:
        raise L.OcoccError(f'{what}: a layout of {int(total)} cells')
    if not balance and int(cap) > 0:
        raise L.OcoccError(f'{what}: cap > 0 with balance == 0: the weighted draw is not built (balance=True with a cap, '
                           'or balance=False without one)')
    return K, local_xyz.size(0)


def tune_sample(sizes, dims, start, total, voxel_size, local_xyz, pts_roi, row_seeds, row_keep=None,
                scale_wlh=[1.0, 1.0, 1.0], offset_wlh=[0.0, 0.0, 0.0], balance=True, cap=-1):
    """The observation sample one online step tunes its shape latents against, from the flat cell list of
    dense_grid_layout (``sizes`` are its enlarged sizes: scale_wlh and offset_wlh are already in them and are taken for
    the symmetry with occ_frame_select only) and the step's pooled points ``local_xyz`` [M, 3] (box frame, after the
    turn of sample_observation), ``pts_roi`` [M].  Per RoI r with k cells, npos of them hit by a point, nneg = k - npos:

        row_keep[r] == 0             no rows (no pooled point: no observation, no tuning)
        balance False                every cell in grid order, label = observed (cap must be <= 0)
        npos == 0                    cell 0 with label 0            nneg == 0      no rows
        npos <= nneg                 the observed cells and the npos free cells of smallest (key, cell)
        npos > nneg > 0              the observed cells, every free cell npos // nneg times and the npos % nneg free
                                     cells of smallest (key, cell) once more (stratified: the reference draws npos times
                                     with replacement)

    in grid order, copies adjacent; more than ``cap`` > 0 rows: the cap rows of smallest (cap key, list position).  The
    keys are the integers of csrc/tune_rng.hpp from ``row_seeds`` [K] int64 (tune_row_seed).  Returns (xyz [S, 3] f32 the
    cell centres, bit for bit dense_grid_cells'; labels [S] int32; index [S] int32, non-decreasing; weights [S] f32 =
    1 / rows of the RoI; counts per RoI as a list of int).  One memset and one mark launch (ococc_occ_frame_mark), one
    count launch, one read-back of the counts, one fill launch (csrc/tune_sample.hip).  ``tune_sample_aten`` is the same
    result, bit for bit, as a torch operator chain: what OCOCC_TUNE_SAMPLE_KERNEL=0 runs."""
    from .. import _lib as L
    K, M = _tune_sample_shapes(L, 'tune_sample', sizes, dims, start, total, local_xyz, pts_roi, row_seeds, row_keep,
                               balance, cap)
    if not TUNE_SAMPLE_KERNEL:
        return tune_sample_aten(sizes, dims, start, total, voxel_size, local_xyz, pts_roi, row_seeds, row_keep,
                                scale_wlh, offset_wlh, balance, cap)
    L.require_device(sizes, dims, start, local_xyz, pts_roi, row_seeds, row_keep)
    dev = sizes.device
    n = int(total)
    if K == 0:
        return (L.empty((0, 3), torch.float32, dev), L.empty((0,), torch.int32, dev), L.empty((0,), torch.int32, dev),
                L.empty((0,), torch.float32, dev), [])
    sizes, dims, start, row_seeds = sizes.contiguous(), dims.contiguous(), start.contiguous(), row_seeds.contiguous()
    seen = L.empty((n,), torch.uint8, dev)
    L.check(L.lib.ococc_occ_frame_mark(L.ptr(local_xyz.contiguous()), L.ptr(pts_roi.to(torch.int32).contiguous()), M,
                                       L.ptr(sizes), L.ptr(dims), L.ptr(start), K, float(voxel_size), L.ptr(seen), n,
                                       L.stream()), 'occ_frame_mark')
    if row_keep is not None:
        row_keep = row_keep.contiguous().view(torch.uint8) if row_keep.dtype == torch.bool else row_keep.contiguous()
    counts = L.empty((K,), torch.int32, dev)
    plan = L.empty((K, 4), torch.int64, dev)
    L.check(L.lib.ococc_tune_sample_count(L.ptr(seen), n, L.ptr(start), K, L.ptr(row_seeds), L.ptr(row_keep), int(bool(balance)),
                                          int(cap), L.ptr(counts), L.ptr(plan), L.stream()), 'tune_sample_count')
    host = counts.tolist()   # the one read-back
    if min(host) < 0:
        raise L.OcoccError(f'tune_sample: start is not the ascending prefix table of a layout of {n} cells (or a RoI '
                           f'holds more than 2^30 cells): RoI {host.index(min(host))}')
    S = sum(host)
    xyz, labels = L.empty((S, 3), torch.float32, dev), L.empty((S,), torch.int32, dev)
    index, weights = L.empty((S,), torch.int32, dev), L.empty((S,), torch.float32, dev)
    L.check(L.lib.ococc_tune_sample_fill(L.ptr(seen), n, L.ptr(start), K, L.ptr(sizes), L.ptr(dims), float(voxel_size),
                                         L.ptr(row_seeds), L.ptr(counts), L.ptr(plan), L.ptr(xyz), L.ptr(labels),
                                         L.ptr(index), L.ptr(weights), S, L.stream()), 'tune_sample_fill')
    return xyz, labels, index, weights, host


def tune_sample_aten(sizes, dims, start, total, voxel_size, local_xyz, pts_roi, row_seeds, row_keep=None,
                     scale_wlh=[1.0, 1.0, 1.0], offset_wlh=[0.0, 0.0, 0.0], balance=True, cap=-1):
    """``tune_sample`` as an operator chain on any device, bit for bit: the keys through int64 arithmetic, the orders
    through stable argsorts of (RoI << 32 | key), the copies through repeat_interleave.  What the CPU tests run, what
    OCOCC_TUNE_SAMPLE_KERNEL=0 selects and what the kernels are timed against."""
    from .. import _lib as L
    K, M = _tune_sample_shapes(L, 'tune_sample_aten', sizes, dims, start, total, local_xyz, pts_roi, row_seeds, row_keep,
                               balance, cap)
    dev = sizes.device
    n, cap = int(total), int(cap)
    i32, i64 = torch.int32, torch.long
    if K == 0:
        return (sizes.new_zeros((0, 3)), torch.zeros((0,), dtype=i32, device=dev), torch.zeros((0,), dtype=i32, device=dev),
                sizes.new_zeros((0,)), [])
    k = start[1:] - start[:-1]
    if int(start[0]) != 0 or int(start[-1]) != n or bool((k < 0).any()):
        raise L.OcoccError(f'tune_sample_aten: start is not the ascending prefix table of a layout of {n} cells')
    roi = torch.arange(K, device=dev)
    box = torch.repeat_interleave(roi, k, output_size=n)
    local = torch.arange(n, device=dev) - start[box]
    if M:
        seen = _observed_aten(sizes, dims, start, n, voxel_size, local_xyz, pts_roi)
    else:
        seen = torch.zeros(n, dtype=torch.bool, device=dev)
    keep = torch.ones(K, dtype=torch.bool, device=dev) if row_keep is None else row_keep != 0
    zeros = lambda: torch.zeros(K, dtype=i64, device=dev)
    if not balance:
        mult = keep[box].to(i64)
    else:
        npos = zeros().index_add_(0, box, seen.to(i64))
        nneg = k - npos
        drawn = keep & (npos > 0) & (nneg > 0)
        small = npos <= nneg
        div = nneg.clamp_min(1)
        q = torch.where(small, npos, npos % div)
        rep = torch.where(small, torch.zeros_like(npos), npos // div)
        mult = (seen & drawn[box]).to(i64)
        fi = torch.nonzero(~seen & drawn[box]).squeeze(1)     # the free cells of the RoIs that draw, in cell order
        fb = box[fi]
        nfree = torch.where(drawn, nneg, torch.zeros_like(nneg))
        rank = _rank_in_group(fb, _tune_key(row_seeds[fb], local[fi]), torch.cumsum(nfree, 0) - nfree)
        mult[fi] = rep[fb] + (rank < q[fb]).to(i64)
        first = keep & (npos == 0) & (k > 0)
        mult[start[:-1][first]] = 1
    rows = torch.repeat_interleave(torch.arange(n, device=dev), mult)
    rbox = box[rows]
    cnt = zeros().index_add_(0, rbox, torch.ones_like(rbox))
    if cap > 0:
        over = cnt > cap
        pos = torch.arange(rows.numel(), device=dev) - (torch.cumsum(cnt, 0) - cnt)[rbox]
        ci = torch.nonzero(over[rbox]).squeeze(1)
        cb = rbox[ci]
        ncap = torch.where(over, cnt, torch.zeros_like(cnt))
        rank = _rank_in_group(cb, _tune_key(row_seeds[cb] ^ _i64(TUNE_CAP_SALT), pos[ci]), torch.cumsum(ncap, 0) - ncap)
        kept = torch.ones(rows.numel(), dtype=torch.bool, device=dev)
        kept[ci] = rank < cap
        rows, rbox = rows[kept], rbox[kept]
        cnt = cnt.clamp_max(cap)
    d = dims.long()[rbox]
    loc = local[rows]
    coors = torch.stack([loc // (d[:, 1] * d[:, 2]), (loc // d[:, 2]) % d[:, 1], loc % d[:, 2]], 1)
    xyz = coors.to(torch.float) * voxel_size + (-sizes / 2)[rbox] + voxel_size / 2   # dense_voxel_centers_batched's
    weights = (torch.ones(K, dtype=torch.float32, device=dev) / cnt.to(torch.float32))[rbox]
    return xyz, seen[rows].to(i32), rbox.to(i32), weights, cnt.tolist()


# ---------------------------------------------------------------------------------------------------------------------
# occupancy-enhanced scene cloud (csrc/occ_merge.hip)
# 0: occ_merge runs the operator chain occ_merge_aten instead of the kernels
OCC_MERGE_KERNEL = os.environ.get('OCOCC_OCC_MERGE_KERNEL', '1') != '0'


def merge_use_dim(use_dim):
    """``use_dim`` as a tuple of column indices: an int n means range(n), as the reference's points_use_dim"""
    if isinstance(use_dim, bool):
        raise ValueError(f'use_dim is an int or a list of column indices, not {use_dim!r}')
    if isinstance(use_dim, int):
        return tuple(range(use_dim))
    return tuple(int(v) for v in use_dim)


MERGE_MAX_FRAMES = 65535     # the limit of scene_rows.scene_steps_rows


def _occ_merge_shapes(L, what, points, occ, counts, use_dim, row_score, flags, frames=None):
    """(N, C, M, R, use_dim as a tuple, counts as a list of int, frames) of the inputs of occ_merge(_frames) and their
    ``_aten`` chains, or OcoccError; ``frames`` None (one cloud) or (cloud_sizes, frame_rows), returned as lists of int."""
    if points.dtype != torch.float32 or points.dim() != 2:
        raise L.OcoccError(f'{what}: points {tuple(points.shape)} {points.dtype} are not f32 [N, C]')
    if occ.dtype != torch.float32 or occ.dim() != 2 or occ.size(1) != 4:
        raise L.OcoccError(f'{what}: occ {tuple(occ.shape)} {occ.dtype} is not f32 [M, 4] (x, y, z, value)')
    N, C, M = points.size(0), points.size(1), occ.size(0)
    dim = merge_use_dim(use_dim)
    if not 3 <= len(dim) <= 16 or min(dim) < 0 or max(dim) >= C:
        raise L.OcoccError(f'{what}: use_dim {dim!r} is not 3 to 16 columns of a cloud with {C} (x, y, z first)')
    counts = [int(c) for c in counts]
    if any(c < 0 for c in counts) or sum(counts) != M:
        raise L.OcoccError(f'{what}: counts {counts if len(counts) <= 8 else counts[:8] + ["..."]} do not sum to the {M} rows of occ')
    R = len(counts)
    if row_score is not None and (row_score.dtype != torch.float32 or tuple(row_score.shape) != (R,)):
        raise L.OcoccError(f'{what}: row_score {tuple(row_score.shape)} {row_score.dtype} is not f32 [{R}]')
    if flags is not None and (flags.dtype != torch.uint8 or tuple(flags.shape) != (M,)):
        raise L.OcoccError(f'{what}: flags {tuple(flags.shape)} {flags.dtype} are not uint8 [{M}]')
    if frames is not None:
        sizes, frame_rows = frames = [int(v) for v in frames[0]], [int(v) for v in frames[1]]
        F = len(sizes)
        if F > MERGE_MAX_FRAMES:
            raise L.OcoccError(f'{what}: {F} clouds, at most {MERGE_MAX_FRAMES} per call')
        if any(s < 0 for s in sizes) or sum(sizes) != N:
            raise L.OcoccError(f'{what}: cloud_sizes {sizes if F <= 8 else sizes[:8] + ["..."]} must be >= 0 and sum to the {N} points given')
        if len(frame_rows) != R or any(not 0 <= f < F for f in frame_rows):
            raise L.OcoccError(f'{what}: frame_rows must hold the cloud 0..{F - 1} of each of the {R} rows of counts, got '
                               f'{len(frame_rows)} values' + (f' from {min(frame_rows)} to {max(frame_rows)}' if frame_rows else ''))
    return N, C, M, R, dim, counts, frames


def occ_merge(points, occ, counts, use_dim=(0, 1, 2, 3, 4), row_score=None, flags=None, drop_observed=False,
              score_threshold=0.0):
    """The occupancy-enhanced cloud of a frame, what LoadPointsAndOccPredFromFile builds from files
    (mmdet3d/datasets/pipelines/occ_pinelines.py:585-715), from tensors on the device: ``points`` [N, C] f32 the scene
    cloud, ``occ`` [M, 4] f32 (x, y, z, value) and ``counts`` (a host list, the rows of ``occ`` per object) as
    occ_frame_select returns them.  Returns (merged [N + K, D + 2] f32, the survivors per object as a list of int):

        row i < N    points[i, use_dim], then 0, 0
        row N + k    the k-th surviving cell in input order: x, y, z, D - 3 zeros, its score, 1

    The score of a cell is ``row_score[object]`` (f32 [R]) or, without it, column 3 of the cell -- the exported files
    carry the object's score there.  A cell survives iff score > score_threshold in f32 (strict, as
    ``occ_points[:, -1] > self.score_threshold``; a NaN score never survives) and, with ``flags`` (uint8 [M], bit 1: a real
    point of the frame fell into the cell) and ``drop_observed``, its bit 1 is clear.  Values are copied bit for bit.
    One table and one count launch, one cumsum, ONE read-back (the survivors per object; K is their sum), one fill launch
    that also copies the real rows (csrc/occ_merge.hip); without cells the count launches and the read-back are skipped.
    ``occ_merge_aten`` is the same result as a torch operator chain: what OCOCC_OCC_MERGE_KERNEL=0 runs."""
    return _occ_merge(points, occ, counts, None, use_dim, row_score, flags, drop_observed, score_threshold)


def occ_merge_aten(points, occ, counts, use_dim=(0, 1, 2, 3, 4), row_score=None, flags=None, drop_observed=False,
                   score_threshold=0.0):
    """``occ_merge`` as an operator chain on any device, bit for bit the same rows: a column index, a compare, a boolean
    index, zero / one columns and two ``cat``.  What OCOCC_OCC_MERGE_KERNEL=0 selects and what the kernels are timed
    against."""
    from .. import _lib as L
    N, C, M, R, dim, counts, _ = _occ_merge_shapes(L, 'occ_merge_aten', points, occ, counts, use_dim, row_score, flags)
    dev = points.device
    D = len(dim)
    head = torch.cat([points[:, list(dim)], points.new_zeros((N, 2))], 1)
    if M == 0:
        return head, [0] * R
    row = torch.repeat_interleave(torch.arange(R, device=dev), torch.tensor(counts, device=dev), output_size=M)
    score = row_score[row] if row_score is not None else occ[:, 3]
    keep = score > torch.full((), float(score_threshold), dtype=torch.float32, device=dev)
    if flags is not None and drop_observed:
        keep = keep & ((flags & 2) == 0)
    tail = torch.cat([occ[keep, :3], occ.new_zeros((int(keep.sum()), D - 3)), score[keep][:, None]], 1)
    tail = torch.cat([tail, torch.ones_like(tail[:, :1])], 1)
    return torch.cat([head, tail], 0), torch.bincount(row[keep], minlength=R).tolist()


def _prefix(values):
    out = [0]
    for v in values:
        out.append(out[-1] + v)
    return out


def merged_offsets(cloud_sizes, frame_rows, kept):
    """offsets [F + 1] of the segments of occ_merge_frames: the rows of a frame's cloud and the survivors of its rows"""
    rows = list(cloud_sizes)
    for f, k in zip(frame_rows, kept):
        rows[f] += k
    return _prefix(rows)


def occ_merge_frames(points, cloud_sizes, occ, counts, frame_rows, use_dim=(0, 1, 2, 3, 4), row_score=None, flags=None,
                     drop_observed=False, score_threshold=0.0):
    """``occ_merge`` for the clouds of F sensor frames in one call (TrackletRoIHeadOCC.simple_test_scene_steps_merged):
    ``points`` [N, C] f32 the F clouds back to back, ``cloud_sizes`` their F lengths (ints on the host); ``occ`` [M, 4],
    ``counts``, ``row_score`` [R], ``flags`` [M] per ROW in the caller's order as in occ_merge, and ``frame_rows``, R ints
    on the host: the cloud 0..F-1 a row belongs to.  The rows need not be grouped by frame (a chunked step has them
    slot-major).

    Returns (merged [N + K, D + 2] f32, offsets, kept): segment f = merged[offsets[f]:offsets[f + 1]] is, byte for byte,
    what occ_merge returns for cloud f and the cells, scores and flags of the rows with frame_rows[i] == f in ascending i;
    ``offsets`` F + 1 ints and ``kept``, the survivors per input row, are host lists.

    The stable frame-major order of the rows is made on the host (scene_rows.frame_major) and goes up with the cell
    prefix, the row frames, the cloud prefix and the frames' first positions in ONE copy; then one table and one count
    launch, one cumsum, ONE read-back (the survivors per row) and one fill launch for any F
    (ococc_occ_merge_frames_count / _fill, csrc/occ_merge.hip): the fill kernel takes the survivors in front of a frame
    from the scan, nothing is uploaded after the read-back.  R == 0 or M == 0 skips the count launches and the read-back;
    F == 0 is an empty [0, D + 2] array with offsets [0].  ``occ_merge_frames_aten`` is the same result as F operator
    chains: what OCOCC_OCC_MERGE_KERNEL=0 runs.

    Reported before any launch (OcoccError): what occ_merge reports, cloud_sizes that hold a negative or do not sum to N,
    more than 65535 clouds, frame_rows of another length than counts or outside 0..F-1."""
    return _occ_merge(points, occ, counts, (cloud_sizes, frame_rows), use_dim, row_score, flags, drop_observed, score_threshold)


def _occ_merge(points, occ, counts, frames, use_dim, row_score, flags, drop_observed, score_threshold):
    """the body of occ_merge (``frames`` None: the table that goes up is the cell prefix, R + 1 integers) and
    occ_merge_frames (``frames`` = (cloud_sizes, frame_rows): five tables in one copy, the ``_frames`` exports, the
    segment offsets in the result)"""
    import ctypes
    from .. import _lib as L
    from ..scene_rows import frame_major
    from ..tracklet import host_index, host_index_many
    what = 'occ_merge' if frames is None else 'occ_merge_frames'
    N, C, M, R, dim, counts, frames = _occ_merge_shapes(L, what, points, occ, counts, use_dim, row_score, flags, frames)
    L.require_device(points, occ, row_score, flags)
    if not OCC_MERGE_KERNEL:
        if frames is None:
            return occ_merge_aten(points, occ, counts, dim, row_score, flags, drop_observed, score_threshold)
        return occ_merge_frames_aten(points, frames[0], occ, counts, frames[1], dim, row_score, flags, drop_observed,
                                     score_threshold)
    dev = points.device
    D = len(dim)
    points, occ = points.contiguous(), occ.contiguous()
    row_score = row_score.contiguous() if row_score is not None else None
    flags = flags.contiguous() if flags is not None and drop_observed else None
    tiles = int(L.lib.ococc_occ_select_max_tiles(M, R))
    tab = [None] * (1 if frames is None else 5)   # the cell prefix; frames: and order, row frames, cloud prefix, firsts
    if M and frames is None:
        tab = [host_index(_prefix(counts), dev)]
    elif M:
        order, first = frame_major(frames[1], len(frames[0]))
        tab = host_index_many([_prefix(counts), order, frames[1], _prefix(frames[0]), first], dev)
    # what the ``_frames`` exports take more: order and row frames after the prefix, the clouds after R
    start, rows_by_frame = L.ptr(tab[0]), [L.ptr(t) for t in tab[1:3]]
    clouds = [] if frames is None else [L.ptr(tab[3]), L.ptr(tab[4]), len(frames[0])]
    score = (L.ptr(row_score), L.ptr(flags), int(flags is not None), float(score_threshold))
    tile_start = scan = None
    kept = [0] * R
    if M:
        tile_start = L.empty((R + 1,), torch.int64, dev)
        tile_counts = L.empty((tiles,), torch.int32, dev)
        row_counts = L.empty((R,), torch.int64, dev)
        L.check(getattr(L.lib, f'ococc_{what}_count')(
            L.ptr(occ), M, start, *rows_by_frame, R, *clouds, *([] if frames is None else [N]), *score, L.ptr(tile_start),
            L.ptr(tile_counts), tiles, L.ptr(row_counts), L.stream()), f'{what}_count')
        scan = torch.cumsum(tile_counts, 0, dtype=torch.int64) - tile_counts
        kept = [int(v) for v in row_counts.tolist()]   # the one read-back
        if min(kept) < 0 and frames is None:
            raise L.OcoccError(f'occ_merge: start is not an ascending table inside [0, {M}]')
        if min(kept) < 0:
            raise L.OcoccError('occ_merge_frames: the tables failed the check on the device: start ascending inside '
                               f'[0, {M}], order inside [0, {R}), frames inside [0, {len(frames[0])}) and non-decreasing '
                               f'along the order, cloud_start ascending from 0 to {N}')
    K = sum(kept)
    merged = L.empty((N + K, D + 2), torch.float32, dev)
    L.check(getattr(L.lib, f'ococc_{what}_fill')(
        L.ptr(points), N, C, (ctypes.c_int32 * D)(*dim), D, L.ptr(occ), M, start, *rows_by_frame, L.ptr(tile_start), R,
        *clouds, *score, L.ptr(scan), tiles, L.ptr(merged), K, L.stream()), f'{what}_fill')
    if frames is None:
        return merged, kept
    return merged, merged_offsets(frames[0], frames[1], kept), kept


def occ_merge_frames_aten(points, cloud_sizes, occ, counts, frame_rows, use_dim=(0, 1, 2, 3, 4), row_score=None, flags=None,
                          drop_observed=False, score_threshold=0.0):
    """``occ_merge_frames`` as an operator chain on any device, the same bytes: occ_merge_aten per frame on the cloud and
    the cells, scores and flags of the frame's rows, and one ``cat``.  What OCOCC_OCC_MERGE_KERNEL=0 selects and what the
    kernels are timed against."""
    from .. import _lib as L
    N, C, M, R, dim, counts, (sizes, frame_rows) = _occ_merge_shapes(
        L, 'occ_merge_frames_aten', points, occ, counts, use_dim, row_score, flags, (cloud_sizes, frame_rows))
    cloud, cell = _prefix(sizes), _prefix(counts)
    parts, kept = [], [0] * R
    for f in range(len(sizes)):
        rows = [i for i in range(R) if frame_rows[i] == f]
        pick = lambda t: None if t is None else (torch.cat([t[cell[i]:cell[i + 1]] for i in rows]) if rows else t[:0])
        score = None if row_score is None else row_score[rows]
        part, k = occ_merge_aten(points[cloud[f]:cloud[f + 1]], pick(occ), [counts[i] for i in rows], dim, score,
                                 pick(flags), drop_observed, score_threshold)
        parts.append(part)
        for i, v in zip(rows, k):
            kept[i] = int(v)
    merged = torch.cat(parts, 0) if parts else points.new_zeros((0, len(dim) + 2))
    return merged, merged_offsets(sizes, frame_rows, kept), kept
