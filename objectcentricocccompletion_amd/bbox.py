"""Box helpers on the hot path -- host mirror of rotation_3d_in_axis
(mmdet3d/core/bbox/structures/utils.py:21-61) and DeltaXYZWLHRBBoxCoder
(mmdet3d/core/bbox/coders/delta_xyzwhlr_bbox_coder.py:8-90).  Tiny elementwise math."""
import math
import os

import torch

from .registry import BBOX_CODERS

# the crop of the ground-truth occupancy export: csrc/gt_occ_crop.hip (0: the ATen chain of crop_gt_occ_aten)
GT_OCC_KERNEL = os.environ.get('OCOCC_GT_OCC_KERNEL', '1') != '0'


def limit_period(val, offset=0.5, period=3.141592653589793):
    return val - torch.floor(val / period + offset) * period


def _rows7(t):
    """a [n, >= 7] f32 device tensor with unit column stride as (tensor, row stride); a copy only if it is not that"""
    if not (t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]):
        t = t.float().contiguous()
    return t, t.stride(0)


def _plain(*tensors):
    """device f32 tensors nobody differentiates through: the single-launch forms apply"""
    return all(t.is_cuda and t.dtype == torch.float32 and not t.requires_grad for t in tensors)


def rotation_3d_in_axis(points, angles, axis=0):
    """points [N,M,3] rotated by angles [N] about `axis`; note the reference multiplies by the
    TRANSPOSED matrix (einsum 'aij,jka->aik'), i.e. a clockwise turn for axis 2."""
    if (axis == 2 or axis == -1) and points.dim() == 3 and points.shape[-1] == 3 and angles.dim() == 1 \
            and angles.shape[0] == points.shape[0] and _plain(points, angles):
        from . import _lib as L   # one launch instead of a dozen (csrc/target_ops.hip)
        p, a = points.contiguous(), angles.contiguous()
        out = torch.empty_like(p)
        L.check(L.lib.ococc_rotate_z_f32(L.ptr(p), L.ptr(a), p.shape[0], p.shape[1], L.ptr(out), L.stream()), 'rotate_z')
        return out
    rot_sin, rot_cos = torch.sin(angles), torch.cos(angles)
    ones, zeros = torch.ones_like(rot_cos), torch.zeros_like(rot_cos)
    if axis == 1:
        rows = [[rot_cos, zeros, -rot_sin], [zeros, ones, zeros], [rot_sin, zeros, rot_cos]]
    elif axis == 2 or axis == -1:
        rows = [[rot_cos, -rot_sin, zeros], [rot_sin, rot_cos, zeros], [zeros, zeros, ones]]
    elif axis == 0:
        rows = [[zeros, rot_cos, -rot_sin], [zeros, rot_sin, rot_cos], [ones, zeros, zeros]]
    else:
        raise ValueError(f'axis should in range [0, 1, 2], got {axis}')
    rot_mat_T = torch.stack([torch.stack(r) for r in rows])
    return torch.einsum('aij,jka->aik', (points, rot_mat_T))


def points_box_to_box(xyz, from_boxes, to_boxes):
    """xyz [N, M, 3] given in the (gravity-centred) frame of from_boxes[i] -> the frame of to_boxes[i]: the chain of
    ococc_bbox_head.py:1279-1290 / 714-724 (GT-box frame -> ego frame -> RoI frame); boxes [N, >= 7]."""
    if xyz.dim() == 3 and xyz.shape[-1] == 3 and from_boxes.shape[0] == xyz.shape[0] == to_boxes.shape[0] \
            and _plain(xyz, from_boxes, to_boxes) and from_boxes.shape[1] >= 7 and to_boxes.shape[1] >= 7:
        from . import _lib as L
        p = xyz.contiguous()
        (fb, ldf), (tb, ldt) = _rows7(from_boxes), _rows7(to_boxes)
        out = torch.empty_like(p)
        L.check(L.lib.ococc_points_box_to_box_f32(L.ptr(p), L.ptr(fb), ldf, L.ptr(tb), ldt, p.shape[0], p.shape[1], L.ptr(out),
                                                  L.stream()), 'points_box_to_box')
        return out
    xyz = rotation_3d_in_axis(xyz, from_boxes[:, 6], axis=2)
    xyz += from_boxes[..., None, 0:3]
    xyz[..., 2] += from_boxes[:, None, 5] / 2   # voxel centres are gravity centred
    xyz -= to_boxes[..., None, :3]
    xyz[..., 2] -= to_boxes[:, None, 5] / 2
    return rotation_3d_in_axis(xyz, -(to_boxes[:, 6]), axis=2)


def gt_occ_crop_trig(gt_boxes, roi_boxes):
    """(cos, sin) of the GT yaw and of the RoI's ``rot_angle`` as check_pt_in_box3d takes it
    (mmdet3d/ops/roiaware_pool3d/src/points_in_boxes_cuda.cu:24-32): float(rz + pi / 2), the sum in double."""
    ang = (roi_boxes[:, 6].double() + math.pi / 2).float()
    return torch.cos(gt_boxes[:, 6]), torch.sin(gt_boxes[:, 6]), torch.cos(ang), torch.sin(ang)


def _gt_occ_points_mask(cells, gt_boxes, roi_boxes, trig=None):
    """points [N, K, 3] and inside mask [N, K] of crop_gt_occ_aten: element-wise products and sums only, so every
    rounding is defined (an einsum's is not) and is what csrc/gt_occ_crop.hip does"""
    cg, sg, ca, sa = (t[:, None] for t in (trig if trig is not None else gt_occ_crop_trig(gt_boxes, roi_boxes)))
    x, y, z = cells[None, :, 0], cells[None, :, 1], cells[None, :, 2]
    g, r = gt_boxes[:, None, :], roi_boxes[:, None, :]
    # tracklet_roi_head_occ.py:665-670: rotation_3d_in_axis(axis=2) (the transposed matrix), + centre, z + h / 2
    px = (x * cg + y * sg) + g[..., 0]
    py = (-x * sg + y * cg) + g[..., 1]
    pz = (z + g[..., 2]) + g[..., 5] / 2
    # check_pt_in_box3d: |z - cz| > h / 2 is outside (the faces are inside); the four side comparisons are strict
    hh = r[..., 5] / 2
    dz, dx, dy = pz - (r[..., 2] + hh), px - r[..., 0], py - r[..., 1]
    lx = dx * ca + dy * (-sa)
    ly = dx * sa + dy * ca
    hl, hw = r[..., 4] / 2, r[..., 3] / 2
    inside = ~(dz.abs() > hh) & (lx > -hl) & (lx < hl) & (ly > -hw) & (ly < hw)
    return torch.stack([px, py, pz], -1), inside


def crop_gt_occ_aten(cells, gt_boxes, roi_boxes, trig=None):
    """The ground-truth branch of the reference's save_occ_from_tracklet, operator by operator
    (tracklet_roi_head_occ.py:661-689): cells [K, 3] (occupied label cells, gravity centres in the GT box frame) are
    moved into the LiDAR frame of each of the N frames by gt_boxes [N, >= 7] (x, y, z_bottom, w, l, h, yaw) and those
    inside roi_boxes[n] (points_in_boxes_gpu, i.e. check_pt_in_box3d) are kept: a list of N tensors [m_n, 3], cell order
    kept.  ``trig``: (cos_gt, sin_gt, cos_roi, sin_roi) [N] each instead of gt_occ_crop_trig's.  A boolean index, i.e. a
    host synchronisation, per frame: the comparator of crop_gt_occ_packed, and what CPU tensors and
    OCOCC_GT_OCC_KERNEL=0 run."""
    cells, gt_boxes, roi_boxes = cells.float().reshape(-1, 3), gt_boxes.float(), roi_boxes.float()
    pts, inside = _gt_occ_points_mask(cells, gt_boxes, roi_boxes, trig)
    return [pts[n][inside[n]] for n in range(gt_boxes.size(0))]


def gt_occ_crop_kernels(cells, gt_boxes, roi_boxes, cos_gt, sin_gt, cos_roi, sin_roi, values=None):
    """csrc/gt_occ_crop.hip with the cos / sin arrays passed in: (packed [M, 4] f32 on the device, counts per frame as a
    list of int).  One count launch, one cumsum, one fill launch; the one read-back is the per-frame counts."""
    from . import _lib as L
    L.require_device(cells, gt_boxes, roi_boxes, cos_gt, sin_gt, cos_roi, sin_roi, values)
    if cells.dtype != torch.float32 or cells.dim() != 2 or cells.size(1) != 3:
        raise L.OcoccError(f'gt_occ_crop: cells {tuple(cells.shape)} {cells.dtype} are not f32 [K, 3]')
    N, K, dev = gt_boxes.size(0), cells.size(0), cells.device
    if gt_boxes.dim() != 2 or roi_boxes.dim() != 2 or roi_boxes.size(0) != N or gt_boxes.size(1) < 7 or roi_boxes.size(1) < 7:
        raise L.OcoccError(f'gt_occ_crop: boxes {tuple(gt_boxes.shape)} / {tuple(roi_boxes.shape)} are not [N, >= 7] both')
    trig = [cos_gt, sin_gt, cos_roi, sin_roi] + ([values] if values is not None else [])
    if any(t.dtype != torch.float32 or t.numel() != N for t in trig):
        raise L.OcoccError(f'gt_occ_crop: cos / sin / values are not f32 [{N}] each')
    if N == 0 or K == 0:
        return L.empty((0, 4), torch.float32, dev), [0] * N
    cells = cells.contiguous()
    (gb, ldg), (rb, ldr) = _rows7(gt_boxes), _rows7(roi_boxes)
    trig = [t.contiguous().view(-1) for t in trig]
    tiles = int(L.lib.ococc_gt_occ_crop_tiles(N, K))
    boxes = (L.ptr(cells), K, L.ptr(gb), ldg, L.ptr(rb), ldr, N, *(L.ptr(t) for t in trig[:4]))
    return L.count_scan_fill(
        tiles, N, 4, dev,
        lambda tile_counts, frame_counts: L.check(L.lib.ococc_gt_occ_crop_count(
            *boxes, L.ptr(tile_counts), tiles, L.ptr(frame_counts), L.stream()), 'gt_occ_crop_count'),
        lambda scan, out, M: L.check(L.lib.ococc_gt_occ_crop_fill(
            *boxes, L.ptr(scan), tiles, L.ptr(trig[4]) if values is not None else None, L.ptr(out), M, L.stream()),
            'gt_occ_crop_fill'))[:2]


def crop_gt_occ_packed(cells, gt_boxes, roi_boxes, values=None):
    """crop_gt_occ_aten as ONE array: (packed [M, 4] f32: the kept cells of frame 0, then of frame 1, ... in the LiDAR
    frame, ``values[n]`` (1 without values) in column 3; counts per frame as a list of int), bit for bit
    ``torch.cat(crop_gt_occ_aten(...))``.  On the kernels of csrc/gt_occ_crop.hip: one read-back (the counts); the
    device-to-host copy of the packed array is the caller's.  CPU tensors and OCOCC_GT_OCC_KERNEL=0 take the ATen chain."""
    cells, gt_boxes, roi_boxes = cells.float().reshape(-1, 3), gt_boxes.float(), roi_boxes.float()
    if values is not None:
        values = values.to(device=cells.device, dtype=torch.float32).view(-1)
    if GT_OCC_KERNEL and cells.is_cuda:
        return gt_occ_crop_kernels(cells, gt_boxes, roi_boxes, *gt_occ_crop_trig(gt_boxes, roi_boxes), values=values)
    parts = crop_gt_occ_aten(cells, gt_boxes, roi_boxes)
    counts = [int(p.size(0)) for p in parts]
    col = [p.new_ones((p.size(0), 1)) if values is None else values[n].expand(p.size(0), 1) for n, p in enumerate(parts)]
    packed = torch.cat([torch.cat([p, c], 1) for p, c in zip(parts, col)], 0) if parts else cells.new_zeros((0, 4))
    return packed, counts


def box_corners(boxes):
    """[N, 7+] (x, y, z_bottom, dx, dy, dz, yaw) -> [N, 8, 3], the corner order of LiDARInstance3DBoxes.corners
    (mmdet3d/core/bbox/structures/lidar_box3d.py:54-92): (x0y0z0, x0y0z1, x0y1z1, x0y1z0, x1y0z0, x1y0z1, x1y1z1, x1y1z0)
    about the bottom centre, turned about z with rotation_3d_in_axis."""
    unit = boxes.new_tensor([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]])
    unit = unit - boxes.new_tensor([0.5, 0.5, 0.0])
    corners = boxes[:, 3:6].reshape(-1, 1, 3) * unit[None]
    return rotation_3d_in_axis(corners, boxes[:, 6], axis=2) + boxes[:, :3].reshape(-1, 1, 3)


@BBOX_CODERS.register_module()
class DeltaXYZWLHRBBoxCoder(object):
    """(x, y, z_bottom, w, l, h, r) deltas normalised by the anchor diagonal / height."""

    def __init__(self, code_size=7):
        self.code_size = code_size

    @staticmethod
    def encode(src_boxes, dst_boxes):
        xa, ya, za, wa, la, ha, ra, *cas = torch.split(src_boxes, 1, dim=-1)
        xg, yg, zg, wg, lg, hg, rg, *cgs = torch.split(dst_boxes, 1, dim=-1)
        cts = [g - a for g, a in zip(cgs, cas)]
        za = za + ha / 2
        zg = zg + hg / 2
        diagonal = torch.sqrt(la ** 2 + wa ** 2)
        return torch.cat([(xg - xa) / diagonal, (yg - ya) / diagonal, (zg - za) / ha, torch.log(wg / wa),
                          torch.log(lg / la), torch.log(hg / ha), rg - ra, *cts], dim=-1)

    @staticmethod
    def decode(anchors, deltas):
        xa, ya, za, wa, la, ha, ra, *cas = torch.split(anchors, 1, dim=-1)
        xt, yt, zt, wt, lt, ht, rt, *cts = torch.split(deltas, 1, dim=-1)
        za = za + ha / 2
        diagonal = torch.sqrt(la ** 2 + wa ** 2)
        xg, yg, zg = xt * diagonal + xa, yt * diagonal + ya, zt * ha + za
        lg, wg, hg = torch.exp(lt) * la, torch.exp(wt) * wa, torch.exp(ht) * ha
        zg = zg - hg / 2
        cgs = [t + a for t, a in zip(cts, cas)]
        return torch.cat([xg, yg, zg, wg, lg, hg, rt + ra, *cgs], dim=-1)


def build_bbox_coder(cfg):
    return BBOX_CODERS.build(cfg)
