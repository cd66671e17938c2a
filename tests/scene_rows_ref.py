"""csrc/scene_rows.hip restated in numpy, for the tests: membership in the kernel's f32 operation order (every product and
sum rounded to f32 on its own: the device may fuse a multiply-add, so a point within an ulp of a face can differ -- the GPU
tests compare memberships with the existing crop kernel, not with this), the transform in float64 (the kernel's f32 result
is held to a rounding bound around it), the even pick in Python ints."""
import numpy as np

F = np.float32


def even_pick(m, cap):
    """[(member j, its place in the box)] of a box of m members under a cap of ``cap`` rows (cap <= 0: none)"""
    if cap <= 0 or m <= cap:
        return [(j, j) for j in range(m)]
    return [(j, j * cap // m) for j in range(m) if (j + 1) * cap // m > j * cap // m]


def in_box(xyz, box):
    """xyz [N, 3] f32, box [7] f32 (x, y, z_bottom, w, l, h, yaw; already enlarged) -> bool [N], tracklet_crop_kernel's
    test: height, conservative radius, BEV with strict inequalities.  A NaN x or y fails; a NaN z passes the height test,
    written ``!(|dz| > h/2)``, as it does there."""
    xyz, box = np.asarray(xyz, F), np.asarray(box, F)
    hh, hl, hw = box[5] * F(0.5), box[4] * F(0.5), box[3] * F(0.5)
    rot = F(np.float64(box[6]) + 1.5707963267948966)
    ca, sa = F(np.cos(rot)), F(np.sin(rot))
    cz = box[2] + hh
    r2 = (hl * hl + hw * hw) * F(1.001) + F(1e-6)
    with np.errstate(invalid='ignore', over='ignore'):
        dx, dy = xyz[:, 0] - box[0], xyz[:, 1] - box[1]
        inside = ~(np.abs(xyz[:, 2] - cz) > hh) & ~(dx * dx + dy * dy > r2)
        lx, ly = dx * ca + dy * (-sa), dx * sa + dy * ca
        return inside & (lx > -hl) & (lx < hl) & (ly > -hw) & (ly < hw)


def transform64(xyz, m12):
    """xyz [M, 3] through the row-major 3x4 matrix m12 [12] (or one per row, [M, 12]) in float64"""
    m = np.asarray(m12, np.float64).reshape(-1, 3, 4)
    p = np.asarray(xyz, np.float64)
    return (m[:, :, :3] * p[:, None, :]).sum(-1) + m[:, :, 3]


def transform_bound(xyz, m12):
    """3 * 2^-24 * (|x m0| + |y m1| + |z m2| + |m3|) per written coordinate: three roundings (one per fused multiply-add),
    each at most half an ulp of a partial sum that is no larger than the sum of the terms' magnitudes"""
    m = np.abs(np.asarray(m12, np.float64).reshape(-1, 3, 4))
    p = np.abs(np.asarray(xyz, np.float64))
    return 3 * 2.0 ** -24 * ((m[:, :, :3] * p[:, None, :]).sum(-1) + m[:, :, 3])


def in_range(xyz, rng):
    """PointsRangeFilter's rule: strictly inside (x0, y0, z0, x1, y1, z1), compared in f32"""
    xyz, r = np.asarray(xyz, F), np.asarray(rng, F)
    with np.errstate(invalid='ignore'):
        return ((xyz[:, 0] > r[0]) & (xyz[:, 1] > r[1]) & (xyz[:, 2] > r[2]) &
                (xyz[:, 0] < r[3]) & (xyz[:, 1] < r[4]) & (xyz[:, 2] < r[5]))


def scene_rows(points, crop_boxes, transforms=None, rng=None, cap=-1, attr_dims=0, row_feats=None):
    """The two passes on the host -> (xyz [M, 3] f64 (the float64 transform; the input values without one), feats
    [M, A + K] f32, row [M] i64, counts [n] i64 uncapped).  Rows sorted by (box, point index)."""
    points, crop_boxes = np.asarray(points, F), np.asarray(crop_boxes, F)
    n = len(crop_boxes)
    K = 0 if row_feats is None else np.asarray(row_feats).shape[1]
    xyz, feats, row, counts = [], [], [], np.zeros(n, np.int64)
    for b in range(n):
        idx = np.flatnonzero(in_box(points[:, :3], crop_boxes[b]))
        w = points[idx, :3].astype(np.float64) if transforms is None else transform64(points[idx, :3], transforms[b])
        if rng is not None:
            keep = in_range(w.astype(F), rng)       # (the kernel compares its own f32 result: equal away from the faces)
            idx, w = idx[keep], w[keep]
        counts[b] = len(idx)
        sel = [j for j, _ in even_pick(len(idx), cap)]
        xyz.append(w[sel])
        f = [points[idx[sel], 3:3 + attr_dims]]
        if K:
            f.append(np.repeat(np.asarray(row_feats, F)[b:b + 1], len(sel), 0))
        feats.append(np.concatenate(f, 1))
        row.append(np.full(len(sel), b, np.int64))
    cat = lambda parts, shape: np.concatenate(parts, 0) if parts else np.zeros(shape)
    return cat(xyz, (0, 3)), cat(feats, (0, attr_dims + K)).astype(F), cat(row, (0,)).astype(np.int64), counts
