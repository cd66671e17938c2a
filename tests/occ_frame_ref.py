"""What tests/test_occ_frame_cpu.py and tests/test_gpu_occ_frame.py share: a plain numpy restatement, in f32 with
explicit loops, of the completed occupancy of one online step (csrc/occ_frame.hip behind occ_ops.occ_frame_select, the
operator chain occ_ops.occ_frame_select_aten) -- mark, selection, centre, pose, matrix, flags and counts -- and the one
input both suites run it on.

The restatement evaluates no transcendental function: the cos / sin of the yaws and the sigmoid of the logits are inputs
(the caller takes them from torch on the device under test, whose values the kernels are documented to reproduce).
Every np.float32 operation below is one IEEE operation rounded once, which is what ``#pragma clang fp contract(off)``
makes of the kernels' expressions."""
import types

import numpy as np
import torch

F = np.float32
V = 0.2
U = 2.0 ** -24          # unit roundoff of f32
# (scale_wlh, offset_wlh): the layout's enlarged sizes are TARGET under both
ENLARGE = [([1.0, 1.0, 1.0], [0.0, 0.0, 0.0]), ([1.2, 1.0, 1.1], [0.0, 0.0, 0.0])]   # (y scale 1: 2.0 stays exact)
# ENLARGED sizes and the cells they give at a 0.2 m voxel, one RoI per tile shape:
#   0: 2 x 2 x 3 = 12, one short tile; all logits negative, holds points: flag 2 alone
#   1: 16 x 8 x 8 = 1024, exactly one full tile; all logits positive
#   2: 13 x 10 x 8 = 1040, a full tile and a second one of 16 cells (a round that is partly filled); y = 2.0 is an exact
#      multiple of the voxel: a point on its upper face has index 10 = dim
#   3: 11 x 11 x 17 = 2057, three tiles; the logits at the threshold and its two f32 neighbours live here
#   4: 5 x 4 x 3 = 60, row_keep 0 with positive logits and points: emits nothing
#   5: 4 x 3 x 3 = 36, negative logits, no point: no cell selected
TARGET = [[0.3, 0.3, 0.5], [3.1, 1.5, 1.5], [2.5, 2.0, 1.5], [2.1, 2.1, 3.3], [0.9, 0.7, 0.5], [0.7, 0.5, 0.5]]
CELLS = [12, 1024, 1040, 2057, 60, 36]
FILTERED, UNSEEN, SEEN_ONLY, ALL_POSITIVE = 4, 5, 0, 1


def layout_ref(wlh, scale, offset, voxel):
    """(enlarged sizes [R, 3] f32, dims [R, 3], start [R + 1]) with the arithmetic of occ_ops.dense_grid_layout"""
    R = wlh.shape[0]
    sizes, dims, start = np.zeros((R, 3), F), np.zeros((R, 3), np.int64), np.zeros(R + 1, np.int64)
    for r in range(R):
        for a in range(3):
            sizes[r, a] = F(F(wlh[r, a]) * F(scale[a])) + F(offset[a])
            dims[r, a] = int(np.ceil(F(sizes[r, a]) / F(voxel)))
        start[r + 1] = start[r] + dims[r, 0] * dims[r, 1] * dims[r, 2]
    return sizes, dims, start


def mark_ref(local_xyz, pts_roi, sizes, dims, start, voxel):
    """observed [total] u8: 1 where a point fell into the cell; floor((p - (-size / 2)) / voxel) per axis, a point whose
    index is < 0 or >= dim on any axis marks nothing"""
    seen = np.zeros(int(start[-1]), np.uint8)
    for i in range(local_xyz.shape[0]):
        r = int(pts_roi[i])
        idx, inside = [], True
        for a in range(3):
            lo = F(-sizes[r, a]) / F(2.0)
            q = np.floor(F(F(local_xyz[i, a]) - lo) / F(voxel))
            inside = inside and bool(q >= 0) and bool(q < dims[r, a])
            idx.append(int(q) if np.isfinite(q) else 0)
        if inside:
            seen[start[r] + (idx[0] * dims[r, 1] + idx[1]) * dims[r, 2] + idx[2]] = 1
    return seen


def frame_select_ref(prob, pos_thresh, wlh, scale, offset, voxel, rois, cos, sin, local_xyz, pts_roi, row_keep=None,
                     transforms=None, observed=True):
    """-> namespace(out [N, 4] f32, flags [N] u8, counts [R], seen [total] u8, cell [N] the flat cell id of every row).
    prob [total] f32: the sigmoid of every cell's logit; rois [R, 8] f32 (batch, x, y, z, w, l, h, yaw); cos, sin [R] f32;
    transforms [R, 12] f32 or None."""
    voxel = F(voxel)
    sizes, dims, start = layout_ref(wlh, scale, offset, voxel)
    R = wlh.shape[0]
    seen = mark_ref(local_xyz, pts_roi, sizes, dims, start, voxel)
    used = seen if observed else np.zeros_like(seen)
    out, flags, cell, counts = [], [], [], [0] * R
    half = voxel / F(2.0)
    for r in range(R):
        if row_keep is not None and not row_keep[r]:
            continue
        dy, dz = int(dims[r, 1]), int(dims[r, 2])
        lo = [F(-sizes[r, a]) / F(2.0) for a in range(3)]
        c, s = F(cos[r]), F(sin[r])
        bx, by, bz, hh = F(rois[r, 1]), F(rois[r, 2]), F(rois[r, 3]), F(rois[r, 6]) / F(2.0)
        for i in range(int(start[r]), int(start[r + 1])):
            pred = bool(F(prob[i]) > F(pos_thresh))
            if not (pred or used[i]):
                continue
            k = i - int(start[r])
            ix, iy, iz = k // (dy * dz), (k // dz) % dy, k % dz
            x, y, z = [F(F(F(j) * voxel) + lo[a]) + half for a, j in enumerate((ix, iy, iz))]
            # OccDecoder._to_lidar: x c + y s, -x s + y c, + the bottom centre, z + h / 2
            x, y, z = F(F(x * c) + F(y * s)) + bx, F(F(F(-x) * s) + F(y * c)) + by, F(z + bz) + hh
            if transforms is not None:
                t = transforms[r]
                x, y, z = [F(F(F(F(t[4 * j] * x) + F(t[4 * j + 1] * y)) + F(t[4 * j + 2] * z)) + t[4 * j + 3])
                           for j in range(3)]
            out.append([x, y, z, F(prob[i])])
            flags.append((1 if pred else 0) | (2 if used[i] else 0))
            cell.append(i)
            counts[r] += 1
    return types.SimpleNamespace(out=np.asarray(out, F).reshape(-1, 4), flags=np.asarray(flags, np.uint8), counts=counts,
                                 seen=seen, cell=np.asarray(cell, np.int64))


def matrix_bound(t12, xyz):
    """per coordinate 3u / (1 - 3u) * (|t0 x| + |t1 y| + |t2 z| + |t3|) in float64: the bound of three products and
    three sums; t12 [N, 12], xyz [N, 3] the point the matrix is applied to -> [N, 3]"""
    t = np.abs(t12.astype(np.float64).reshape(-1, 3, 4))
    p = np.abs(xyz.astype(np.float64))
    return 3 * U / (1 - 3 * U) * ((t[:, :, :3] * p[:, None, :]).sum(-1) + t[:, :, 3])


def apply64(t12, xyz):
    """the same f32 matrices applied in float64"""
    t = t12.astype(np.float64).reshape(-1, 3, 4)
    return (t[:, :, :3] * xyz.astype(np.float64)[:, None, :]).sum(-1) + t[:, :, 3]


def yawed_pose(yaw, tx, ty, tz):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([c, -s, 0, tx, s, c, 0, ty, 0, 0, 1, tz], np.float32)


def make_case(enlarge, pos_thresh, seed=23):
    """The input of both suites as CPU tensors: six RoIs (TARGET), logits and about 200 points.
    Logits: random; RoI 1 all positive; RoIs 0 and 5 all negative; RoI 4 positive (and filtered); in RoI 3 several logits
    exactly at the threshold's logit and at its two f32 neighbours.
    Points, in the frames of their boxes: random ones inside RoIs 0, 2, 3 and 4; one on a lower face and one on an upper
    face (of RoI 2's y axis: index 10 = dim, outside); one outside the grid on each axis and side; two in one cell."""
    scale, offset = enlarge
    g = torch.Generator().manual_seed(seed)
    target = torch.tensor(TARGET, dtype=torch.float32)
    wlh = (target - torch.tensor(offset)) / torch.tensor(scale)
    R = wlh.size(0)
    rois = torch.cat([torch.zeros(R, 1), torch.rand(R, 3, generator=g) * 80 - 40, wlh,
                      torch.rand(R, 1, generator=g) * 6.4 - 3.2], 1)
    start = np.cumsum([0] + CELLS)
    total = int(start[-1])
    logits = torch.randn(total, generator=g) * 3
    thr = np.float32(np.log(pos_thresh / (1 - pos_thresh)))
    near = torch.tensor([thr, np.nextafter(thr, np.float32(1)), np.nextafter(thr, np.float32(-1))], dtype=torch.float32)
    at = torch.arange(int(start[3]) + 5, int(start[4]), 37)
    logits[at] = near[torch.arange(at.numel()) % 3]

    def span(r):
        return slice(int(start[r]), int(start[r + 1]))
    logits[span(ALL_POSITIVE)] = logits[span(ALL_POSITIVE)].abs() + 1.0
    logits[span(FILTERED)] = logits[span(FILTERED)].abs() + 1.0
    logits[span(SEEN_ONLY)] = -logits[span(SEEN_ONLY)].abs() - 1.0
    logits[span(UNSEEN)] = -logits[span(UNSEEN)].abs() - 1.0
    xyz, roi = [], []
    for r, n in ((0, 8), (2, 70), (3, 90), (FILTERED, 15)):
        xyz.append((torch.rand(n, 3, generator=g) - 0.5) * target[r] * 0.999)
        roi += [r] * n
    half = target / 2
    special = [(2, [-half[2, 0], 0.05, 0.05]),                      # on the lower x face: index 0
               (2, [0.05, half[2, 1], 0.05]),                       # on the upper y face: index 10 = dim, outside
               (3, [0.31, -0.47, 0.93]), (3, [0.33, -0.45, 0.95])]  # two in one cell
    for a in range(3):
        for side in (-1.0, 1.0):
            p = [0.05, 0.05, 0.05]
            p[a] = side * (float(half[3, a]) + 0.3)
            special.append((3, p))
    xyz.append(torch.tensor([[float(v) for v in p] for _, p in special], dtype=torch.float32))
    roi += [r for r, _ in special]
    keep = torch.ones(R, dtype=torch.uint8)
    keep[FILTERED] = 0
    return types.SimpleNamespace(scale=scale, offset=offset, wlh=wlh, rois=rois, logits=logits, total=total, R=R,
                                 local_xyz=torch.cat(xyz).contiguous(), pts_roi=torch.tensor(roi, dtype=torch.int32),
                                 row_keep=keep, pos_thresh=pos_thresh, thr=float(thr), near=at)


def run_ref(case, prob, cos, sin, row_keep=None, transforms=None, observed=True, points=True):
    """frame_select_ref on a case; prob, cos, sin: torch tensors from the device under test"""
    n = case.local_xyz.size(0) if points else 0
    return frame_select_ref(prob.cpu().numpy(), case.pos_thresh, case.wlh.numpy(), case.scale, case.offset, V,
                            case.rois.numpy(), cos.cpu().numpy(), sin.cpu().numpy(), case.local_xyz.numpy()[:n],
                            case.pts_roi.numpy()[:n], None if row_keep is None else row_keep.cpu().numpy(),
                            None if transforms is None else transforms.cpu().numpy(), observed)
