"""Host mirror of mmdet3d/ops/occ/occ_ops.py: voxel-centre helpers of the implicit
occupancy grid (generate_dense_voxel_centers :5-50, quantize_points :53-93,
jitter_voxel_center :96-100).  Elementwise index math on small tensors."""
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
