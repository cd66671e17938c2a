"""Test data and the float64 restatement for the ground-truth occupancy crop (csrc/gt_occ_crop.hip,
bbox.crop_gt_occ_aten): the reference's branch tracklet_roi_head_occ.py:661-689 with check_pt_in_box3d of
roiaware_pool3d/src/points_in_boxes_cuda.cu:24-49.  Shared by test_gt_occ_crop_cpu.py and test_gpu_gt_occ_crop.py."""
import math

import numpy as np
import torch


def random_case(n, k, seed, dev='cpu'):
    """n GT boxes anywhere within 80 m at any yaw, proposal boxes around them (shifted, resized, turned: part of the
    cells falls outside), k cells spread a little beyond the GT box"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    size = torch.tensor([2.0, 4.6, 1.7]) + u(n, 3) * torch.tensor([0.4, 1.0, 0.4])
    gt = torch.cat([u(n, 2) * 80, u(n, 1) * 4, size, u(n, 1) * math.pi], 1)
    roi = gt + torch.cat([u(n, 3) * 0.5, u(n, 3) * 0.3, u(n, 1) * 0.3], 1)
    cells = u(k, 3) * torch.tensor([1.4, 2.9, 1.1])
    return cells.to(dev), gt.to(dev), roi.to(dev)


def restate_f64(cells, gt, roi):
    """float64: the LiDAR-frame points [N, K, 3], the inside mask [N, K] and the distance of every point to the nearest
    face plane of its RoI [N, K]"""
    c, g, r = (t.double().numpy() for t in (cells, gt, roi))
    cg, sg = np.cos(g[:, 6])[:, None], np.sin(g[:, 6])[:, None]
    x, y, z = c[None, :, 0], c[None, :, 1], c[None, :, 2]
    px = x * cg + y * sg + g[:, None, 0]                      # rotation_3d_in_axis(axis=2): the transposed matrix
    py = -x * sg + y * cg + g[:, None, 1]
    pz = z + g[:, None, 2] + g[:, None, 5] / 2
    ang = r[:, 6] + math.pi / 2
    ca, sa = np.cos(ang)[:, None], np.sin(ang)[:, None]
    dz = pz - (r[:, None, 2] + r[:, None, 5] / 2)
    dx, dy = px - r[:, None, 0], py - r[:, None, 1]
    lx, ly = dx * ca + dy * (-sa), dx * sa + dy * ca
    hl, hw, hh = r[:, None, 4] / 2, r[:, None, 3] / 2, r[:, None, 5] / 2
    inside = ~(np.abs(dz) > hh) & (lx > -hl) & (lx < hl) & (ly > -hw) & (ly < hw)
    dist = np.minimum(np.minimum(np.abs(np.abs(dz) - hh), np.abs(np.abs(lx) - hl)), np.abs(np.abs(ly) - hw))
    return np.stack([px, py, pz], -1), inside, dist


def face_case(dev='cpu'):
    """cos = 1 and sin = 0 on both boxes and dyadic coordinates: every sum is exact, so a cell sits exactly ON a face.
    GT box: bottom centre (8, -4, 1), h 2: the point is (x + 8, y - 4, z + 2).  RoI: bottom centre (8, -4, 0.5),
    w 2, l 4, h 3: gravity centre z 2, so local (x, y, z).  -> cells, boxes, trig, expected keep mask"""
    cells = torch.tensor([[0.0, 0.0, 0.0],       # the centre                    kept
                          [0.5, 0.25, 1.5],      # on the top face               kept
                          [-1.0, -0.5, -1.5],    # on the bottom face            kept
                          [0.5, 0.25, 1.75],     # above the top face            dropped
                          [2.0, 0.0, 0.0],       # on the +x face (l / 2)        dropped
                          [-2.0, 0.5, 0.0],      # on the -x face                dropped
                          [0.0, 1.0, 0.0],       # on the +y face (w / 2)        dropped
                          [1.0, -1.0, 0.5],      # on the -y face                dropped
                          [1.875, 0.875, 1.5],   # inside the sides, on the top  kept
                          [2.0, 1.0, 1.5]])      # an edge of sides and top      dropped
    keep = [True, True, True, False, False, False, False, False, True, False]
    gt = torch.tensor([[8.0, -4.0, 1.0, 2.0, 4.0, 2.0, 0.3]])      # (the yaw columns are not read: trig is passed in)
    roi = torch.tensor([[8.0, -4.0, 0.5, 2.0, 4.0, 3.0, -0.9]])
    one, zero = torch.ones(1), torch.zeros(1)
    trig = tuple(t.to(dev) for t in (one, zero, one, zero))
    return cells.to(dev), gt.to(dev), roi.to(dev), trig, keep
