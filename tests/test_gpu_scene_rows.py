"""Online inference from whole-scene clouds on the MI355X (csrc/scene_rows.hip, scene_rows.scene_step_rows,
TrackletRoIHeadOCC.simple_test_scene_step, tools/online_raw.py).

A. without transform, range and cap the rows are those of the existing crop (ctrl_prep.crop_frames_packed) gathered with
   plain indexing: torch.equal, over the lane / wave-tile / workgroup edges of N and the LDS chunk edges of n.
B. the f32 transform against float64 within 3 * 2^-24 * (|x m0| + |y m1| + |z m2| + |m3|); the identity gives A's bits.
C. the range filter at its faces.   D. the cap against the even pick of the uncapped rows.   E. workspace reuse.
F. the head on two tracklets under ego motion against the same rows built with the existing operators.
G. the replay tool on a synthetic raw tree."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_rows_ref as R        # noqa: E402
from objectcentricocccompletion_amd import _lib as L        # noqa: E402
from objectcentricocccompletion_amd import ctrl_prep        # noqa: E402
from objectcentricocccompletion_amd import scene_rows as S  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 3            # rows behind M in the output buffers of raw_rows: must stay as they were filled


@pytest.fixture(scope='module', autouse=True)
def _generators_as_found():
    """later tests of the suite initialise networks from torch's global generators without seeding them: leave both
    as this module found them"""
    cpu = torch.get_rng_state()
    gpu = torch.cuda.get_rng_state() if torch.cuda.is_available() else None
    yield
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state(gpu)


def raw_rows(points, crop, transforms=None, rng=None, A=0, row_feats=None, cap=-1, ws=None):
    """the two exports called as scene_step_rows calls them, with any K and a caller's workspace; the outputs are PAD rows
    longer than M, filled with a sentinel that must survive"""
    dev = points.device
    N, n = points.size(0), crop.size(0)
    K = 0 if row_feats is None else row_feats.size(1)
    counts = torch.full((n,), -7, dtype=torch.int64, device=dev)
    ws_bytes = int(L.lib.ococc_scene_rows_workspace_bytes(N, n))
    if ws is None:
        ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=dev)
    assert ws.numel() >= ws_bytes
    rng = None if rng is None else L.f6(rng)
    L.check(L.lib.ococc_scene_rows_count(L.ptr(points), N, points.size(1), L.ptr(crop), n, L.ptr(transforms), rng,
                                         L.ptr(counts), L.ptr(ws), ws.numel(), L.stream()), 'count')
    ch = counts.cpu()
    scans = torch.zeros((2, n + 1), dtype=torch.int64)
    scans[0, 1:] = torch.cumsum(ch, 0)
    scans[1, 1:] = torch.cumsum(ch.clamp(max=cap) if cap > 0 else ch, 0)
    M = int(scans[1, -1])
    sd = scans.to(dev)
    xyz = torch.full((M + PAD, 3), -777.0, device=dev)
    feats = torch.full((M + PAD, A + K), -777.0, device=dev)
    row = torch.full((M + PAD,), -777, dtype=torch.int64, device=dev)
    L.check(L.lib.ococc_scene_rows_fill(L.ptr(points), N, points.size(1), L.ptr(crop), n, L.ptr(transforms), rng, A,
                                        L.ptr(row_feats), K, cap, L.ptr(sd[0]), L.ptr(sd[1]), L.ptr(xyz), L.ptr(feats),
                                        L.ptr(row), L.ptr(ws), ws.numel(), L.stream()), 'fill')
    assert bool((xyz[M:] == -777).all()) and bool((feats[M:] == -777).all()) and bool((row[M:] == -777).all())
    return xyz[:M], feats[:M], row[:M], ch


def crop_rows(points, crop, A=0, row_feats=None):
    """the same rows from the EXISTING crop: its indices, plain indexing"""
    dev = points.device
    N, n = points.size(0), crop.size(0)
    counts, idx = ctrl_prep.crop_frames_packed(points, [0, N], crop, [0, n])
    row = torch.repeat_interleave(torch.arange(n), counts).to(dev)
    parts = [points[idx, 3:3 + A]]
    if row_feats is not None:
        parts.append(row_feats[row])
    return points[idx, :3], torch.cat(parts, 1), row, counts


def local_to_xy(box, lx, ly):
    """the kernel's BEV rotation inverted: local (x along l, y along w) -> offsets from the box centre"""
    rot = np.asarray(box)[..., 6].astype(np.float64) + np.pi / 2
    ca, sa = np.cos(rot), np.sin(rot)
    return lx * ca + ly * sa, -lx * sa + ly * ca


def scene(N, n, C, seed):
    """n boxes in a 30 m square -- every third a shifted copy of its neighbour (overlap: one point in several rows), every
    fifth far away (no point) -- and N points, about half of them inside some box, some with NaN / +-inf coordinates"""
    g = np.random.default_rng(seed)
    boxes = np.concatenate([g.uniform(-15, 15, (n, 2)), g.uniform(-1, 1, (n, 1)), g.uniform(1.5, 2.5, (n, 1)),
                            g.uniform(3.5, 5.5, (n, 1)), g.uniform(1.4, 2.0, (n, 1)), g.uniform(-np.pi, np.pi, (n, 1))], 1)
    for b in range(2, n, 3):
        boxes[b] = boxes[b - 1]
        boxes[b, :2] += g.uniform(-0.5, 0.5, 2)
    boxes[4::5, :2] += 500
    pts = np.concatenate([g.uniform(-18, 18, (N, 2)), g.uniform(-1.5, 3.5, (N, 1)), g.random((N, C - 3))], 1)
    if n:
        own = np.array([b for b in range(n) if b % 5 != 4])[g.integers(0, n - n // 5, N)]
        inside = g.random(N) < 0.5
        lx, ly = (g.random(N) - 0.5) * boxes[own, 4] * 1.1, (g.random(N) - 0.5) * boxes[own, 3] * 1.1
        dx, dy = local_to_xy(boxes[own], lx, ly)
        z = boxes[own, 2] + g.random(N) * boxes[own, 5] * 1.1 - 0.05
        pts[inside, :3] = np.stack([boxes[own, 0] + dx, boxes[own, 1] + dy, z], 1)[inside]
    # (no NaN z here: it passes the crop's height test, and torch.equal does not hold between NaNs -- test_range_faces has one)
    for k, (col, v) in enumerate(((0, np.nan), (1, np.inf), (2, -np.inf), (1, np.nan), (2, np.inf), (0, -np.inf))):
        if N > 7 * (k + 1):
            pts[7 * (k + 1), col] = v
    return pts.astype(np.float32), boxes.astype(np.float32)


NS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, 9000]


@pytest.mark.parametrize('N', NS)
def test_rows_equal_the_existing_crop(dev, N):
    """A: every n in {0, 1, 63, 64, 65, 130}, (C, A) in {(3, 0), (5, 2), (6, 2)}, K in {0, 5}"""
    for n in (0, 1, 63, 64, 65, 130):
        for C, A in ((3, 0), (5, 2), (6, 2)):
            pts, boxes = scene(N, n, C, seed=1000 * n + N + C)
            points, boxes = torch.from_numpy(pts).to(dev), torch.from_numpy(boxes).to(dev)
            crop = ctrl_prep.enlarged_boxes(boxes, 0.25)
            scores = torch.linspace(0.1, 0.9, max(n, 1), device=dev)[:n]
            deco = S.decoration(boxes, scores)
            for feats_in in (None, deco):
                want = crop_rows(points, crop, A, feats_in)
                got = raw_rows(points, crop, A=A, row_feats=feats_in)
                for g, w, name in zip(got, want, ('xyz', 'feats', 'row', 'counts')):
                    assert g.shape == w.shape and torch.equal(g, w), (name, N, n, C, feats_in is not None)
                if N >= 1023 and n >= 63:
                    assert int(want[3].sum()) > 0 and int((want[3] == 0).sum()) > 0 and int(want[3].sum()) > int((want[3] > 0).sum())
            if C >= 5:     # the host operator: K = 5, its own enlarged boxes and decoration
                xyz, feats, row, counts = S.scene_step_rows(points, boxes, scores, extra_width=0.25, attr_dims=2)
                want = crop_rows(points, crop, 2, deco)
                assert torch.equal(xyz, want[0]) and torch.equal(feats, want[1]) and torch.equal(row, want[2])
                assert torch.equal(counts, want[3]) and not counts.is_cuda and xyz.shape == (int(counts.sum()), 3)


def test_several_box_chunks_per_workgroup(dev):
    """A, at the one size where it shows: the launch splits the boxes over workgroups until about 512 are in flight, so
    only a cloud of more than 256 workgroups (1 048 576 points) makes a workgroup walk more than one LDS chunk of 64 boxes
    (130 boxes in two spans of 65: chunks of 64 and 1)"""
    pts, boxes = scene(4096 * 256 + 5, 130, 3, seed=77)
    points, crop = torch.from_numpy(pts).to(dev), ctrl_prep.enlarged_boxes(torch.from_numpy(boxes).to(dev), 0.25)
    got, want = raw_rows(points, crop), crop_rows(points, crop)
    assert int(want[3].sum()) > 100000 and all(torch.equal(a, b) for a, b in zip(got, want))
    ident = torch.eye(4, device=dev)[:3].reshape(1, 12).repeat(130, 1).contiguous()
    same = raw_rows(points, crop, transforms=ident, rng=[-1e4, -1e4, -1e4, 1e4, 1e4, 1e4])
    assert all(torch.equal(a, b) for a, b in zip(same, want))


def face_scene(dev):
    """a box with yaw = -pi/2: rot = (float)(yaw + pi/2) = -4.4e-8, cos = 1, so with dy == 0 the local x is dx exactly"""
    f = np.float32
    box = np.array([[10, 5, 1, 2, 4, 2, -np.pi / 2]], f)                      # centre z = 2, l/2 = 2, h/2 = 1
    pts = np.array([[12, 5, 2], [8, 5, 2], [np.nextafter(f(12), f(0)), 5, 2], [np.nextafter(f(8), f(20)), 5, 2],
                    [10, 5, 3], [10, 5, 1], [10, 5, np.nextafter(f(3), f(9))], [10, 5, f(1) - f(2.0 ** -22)]], f)
    return torch.from_numpy(pts).to(dev), torch.from_numpy(box).to(dev), [False, False, True, True, True, True, False, False]


def test_faces_of_a_box(dev):
    """A, crafted to be exact: local x = +-l/2 is outside (strict), z = centre +- h/2 is inside (<=)"""
    points, box, inside = face_scene(dev)
    assert R.in_box(points.cpu().numpy(), box.cpu().numpy()[0]).tolist() == inside
    xyz, _, row, counts = raw_rows(points, box)
    want = crop_rows(points, box)
    assert counts.tolist() == [sum(inside)] and torch.equal(xyz, points[torch.tensor(inside, device=dev)])
    assert torch.equal(xyz, want[0]) and torch.equal(counts, want[3]) and row.tolist() == [0] * sum(inside)


def test_transform_against_float64(dev):
    """B: a different matrix per row (rotation about an oblique axis, translation up to 80 m), overlapping boxes so that one
    point is written through two matrices; every coordinate within the bound of three f32 roundings of the float64 result;
    identity matrices give the untransformed bits"""
    pts, boxes = scene(5000, 66, 5, seed=11)
    points, boxes_d = torch.from_numpy(pts).to(dev), torch.from_numpy(boxes).to(dev)
    crop = ctrl_prep.enlarged_boxes(boxes_d, 0.25)
    g = np.random.default_rng(12)
    mats = np.zeros((66, 3, 4))
    for b in range(66):
        q, _ = np.linalg.qr(g.normal(size=(3, 3)))
        mats[b, :, :3], mats[b, :, 3] = q, g.uniform(-80, 80, 3)
    m32 = torch.from_numpy(mats.reshape(66, 12).astype(np.float32)).to(dev)
    plain = raw_rows(points, crop, A=2)
    xyz, feats, row, counts = raw_rows(points, crop, transforms=m32, A=2)
    assert torch.equal(feats, plain[1]) and torch.equal(row, plain[2]) and torch.equal(counts, plain[3])
    src, rows = plain[0].cpu().numpy(), row.cpu().numpy()
    twice = np.unique(src, axis=0, return_counts=True)[1]
    assert (twice >= 2).sum() > 10, 'no point lies in two boxes'
    m_rows = m32.cpu().numpy().astype(np.float64)[rows]
    err = np.abs(xyz.cpu().numpy().astype(np.float64) - R.transform64(src, m_rows))
    bound = R.transform_bound(src, m_rows)
    print(f'transform: {len(src)} rows, largest error / bound {float((err / bound).max()):.3f}')
    assert (err <= bound).all()
    ident = torch.eye(4, device=dev)[:3].reshape(1, 12).repeat(66, 1).contiguous()
    same = raw_rows(points, crop, transforms=ident, A=2)
    assert all(torch.equal(a, b) for a, b in zip(same, plain))


def test_range_faces(dev):
    """C: identity transforms, PointsRangeFilter's range: a written coordinate of exactly 204.7f or -3.99f is outside, its
    neighbour one ulp inside is a row; counts are the rows' (the range is part of membership in both passes)"""
    f = np.float32
    rng = [-204.7, -204.7, -3.99, 204.7, 204.7, 7.99]
    hi, lo = f(204.7), f(-3.99)
    box = np.array([[204, 0, -5, 4, 4, 4, 0.0], [0, 0, -5, 4, 4, 4, 0.3]], f)          # z from -5 to -1
    pts = np.array([[hi, 0, -2, 1], [np.nextafter(hi, f(0)), 0, -2, 2], [np.nextafter(hi, f(999)), 0, -2, 3],
                    [0, 0, lo, 4], [0, 0, np.nextafter(lo, f(0)), 5], [0, 0, np.nextafter(lo, f(-9)), 6],
                    [0.5, 0.5, -2, 7], [0, 0, np.nan, 8]], f)
    points, crop = torch.from_numpy(pts).to(dev), torch.from_numpy(box).to(dev)
    ident = torch.eye(4, device=dev)[:3].reshape(1, 12).repeat(2, 1).contiguous()
    free = raw_rows(points, crop, A=1)
    assert free[3].tolist() == [3, 5] and free[1][:, 0].tolist() == [1, 2, 3, 4, 5, 6, 7, 8]   # (a NaN z passes the box test)
    for tf in (None, ident):
        xyz, feats, row, counts = raw_rows(points, crop, transforms=tf, rng=rng, A=1)
        assert feats[:, 0].tolist() == [2, 5, 7] and row.tolist() == [0, 1, 1] and counts.tolist() == [1, 2]
        assert torch.equal(xyz, points[[1, 4, 6], :3])
    want = R.scene_rows(pts, box, rng=rng, attr_dims=1)
    assert want[3].tolist() == [1, 2] and want[1][:, 0].tolist() == [2, 5, 7]


@pytest.mark.parametrize('cap', [1, 5, 64])
def test_cap_is_the_even_pick(dev, cap):
    """D: boxes with m = cap - 1, cap, cap + 1 and 3 cap + 7 members, their points interleaved in the cloud with each other
    and with background; the capped rows are the reference pick of the uncapped rows, counts stay uncapped"""
    g = np.random.default_rng(cap)
    ms = [cap - 1, cap, cap + 1, 3 * cap + 7]
    boxes = np.array([[20.0 * b, 0, 0, 2, 4.5, 1.6, 0.4 * b] for b in range(4)], np.float32)
    parts = [np.concatenate([g.uniform(-60, -30, (300, 2)), g.uniform(0, 2, (300, 1))], 1)]
    for b, m in enumerate(ms):
        dx, dy = local_to_xy(boxes[b], (g.random(m) - 0.5) * 4.0, (g.random(m) - 0.5) * 1.6)
        parts.append(np.stack([boxes[b, 0] + dx, boxes[b, 1] + dy, 0.1 + 1.4 * g.random(m)], 1))
    xyz = np.concatenate(parts)
    pts = np.concatenate([xyz, np.arange(len(xyz))[:, None]], 1)[g.permutation(len(xyz))].astype(np.float32)
    points, crop = torch.from_numpy(pts).to(dev), torch.from_numpy(boxes).to(dev)
    deco = S.decoration(crop, torch.ones(4, device=dev))
    full = raw_rows(points, crop, A=1, row_feats=deco)
    got = raw_rows(points, crop, A=1, row_feats=deco, cap=cap)
    assert full[3].tolist() == ms and got[3].tolist() == ms
    first = np.concatenate([[0], np.cumsum(ms)])
    keep = torch.tensor([first[b] + j for b, m in enumerate(ms) for j, _ in R.even_pick(m, cap)], dtype=torch.long, device=dev)
    assert len(keep) == sum(min(m, cap) for m in ms) == got[0].size(0)
    for a, b in zip(got[:3], full[:3]):
        assert torch.equal(a, b[keep])
    xyz2, feats2, row2, counts2 = S.scene_step_rows(points, crop, torch.ones(4, device=dev), extra_width=0.0, attr_dims=1,
                                                    max_points=cap)
    assert torch.equal(xyz2, got[0]) and torch.equal(feats2, got[1]) and torch.equal(row2, got[2]) and counts2.tolist() == ms


def test_workspace_reuse(dev):
    """E: two calls with different inputs through one workspace (the second smaller: the first call's counts stay behind
    it), each its own result; the outputs have exactly M rows (raw_rows checks the rows behind M)"""
    ws = torch.empty((int(L.lib.ococc_scene_rows_workspace_bytes(9000, 70)),), dtype=torch.uint8, device=dev)
    for N, n, seed in ((9000, 70, 21), (3000, 9, 22), (9000, 70, 21)):
        pts, boxes = scene(N, n, 6, seed)
        points, crop = torch.from_numpy(pts).to(dev), ctrl_prep.enlarged_boxes(torch.from_numpy(boxes).to(dev), 0.25)
        got, want = raw_rows(points, crop, A=2, ws=ws), crop_rows(points, crop, 2)
        assert int(want[3].sum()) > 0 and all(torch.equal(a, b) for a, b in zip(got, want))


# --------------------------------------------------------------------------------------------------------------- the head
@pytest.fixture(scope='module')
def model(dev):
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (register)
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    torch.manual_seed(0)
    return DETECTORS.build(ococcnet_model_cfg()).to(dev).eval()


FRAMES, STARTS, SLOTS, EMPTY = 4, (0, 1), (2, 0), (1, 2)      # EMPTY: (tracklet, its frame) without a point in its box


def ego_pose(f):
    a = 0.05 * f
    pose = np.eye(4)
    pose[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    pose[:3, 3] = [1.5 * f, 0.1 * f * f, 0.02 * f]
    return pose


def head_frames():
    """per sensor frame: cloud [N, 5], pose, and the live tracklets' (tracklet, box, score) in the frame's ego frame"""
    g = np.random.default_rng(5)
    sizes = [np.array([2.0, 4.6, 1.6]), np.array([1.9, 4.2, 1.5])]
    frames = []
    for f in range(max(STARTS) + FRAMES):
        live, parts = [], [np.concatenate([g.uniform(-40, -20, (400, 2)), g.uniform(0, 2, (400, 1))], 1)]     # background
        for t, start in enumerate(STARTS):
            k = f - start
            if not 0 <= k < FRAMES:
                continue
            box = np.concatenate([[12 + 0.3 * f, -6 + 12 * t + 0.1 * f, 0.1], sizes[t], [0.02 * f + 0.7 * t]]).astype(np.float32)
            live.append((t, box, np.float32(0.4 + 0.1 * t + 0.05 * k)))
            if (t, k) != EMPTY:
                m = 150
                dx, dy = local_to_xy(box, (g.random(m) - 0.5) * sizes[t][1], (g.random(m) - 0.5) * sizes[t][0])
                parts.append(np.stack([box[0] + dx, box[1] + dy, box[2] + g.random(m) * sizes[t][2]], 1))
        xyz = np.concatenate(parts)
        cloud = np.concatenate([xyz, g.random((len(xyz), 2))], 1)[g.permutation(len(xyz))].astype(np.float32)
        frames.append((cloud, ego_pose(f), live))
    return frames


def test_head_scene_step_matches_the_existing_operators(dev, model):
    """F: two tracklets of 4 frames under ego motion in slots [2, 0] of a three-slot state, the second one frame late (its
    own origin), one (tracklet, frame) without a point in its box, background outside every box.  The same rows built with the
    existing operators -- crop_frames_packed and indexing, the transform as ATen operators in the kernel's order (each
    multiply-add in float64, where the product of two f32 is exact, rounded to f32: a fused multiply-add but for a double
    rounding of probability about 2^-29; ATen's own f32 addcmul rounds the product first, so some coordinates differ in the
    last bit), PointDecoration's expressions, the range mask -- go through simple_test_step on a second state, with
    the SAME fixed-frame boxes (the head's batched float64 mapping, held separately to Tracklet.frame_transform within f32
    rounding of the f32 path, 1e-5).  valid equal; boxes, scores and fused_roi_feats within 2 d0 + 1e-7 relative, d0 = what
    two runs of simple_test_step on identical rows differ by (the step is not bit-reproducible: d0 is the largest distance
    of three more runs from the reference run, printed); boxes_ego of valid rows within the bound of
    three f32 roundings of the float64 inverse map, the invalid row's boxes_ego its input bit for bit."""
    from objectcentricocccompletion_amd.tracklet import Tracklet
    rh = model.roi_head
    cfg = rh.SCENE_ROWS_DEFAULTS
    rng = torch.tensor(cfg['point_cloud_range'], dtype=torch.float32, device=dev)
    state, ref_state, *twin_states = (rh.online_begin(3, dev, cap=FRAMES) for _ in range(5))
    origin = {}
    worst = dict(boxes=0.0, scores=0.0, fused_roi_feats=0.0)
    d0 = dict(worst)
    xyz_equal, feats_equal, seen_invalid = True, True, False
    for f, (cloud, pose, live) in enumerate(head_frames()):
        points = torch.from_numpy(cloud).to(dev)
        boxes = torch.from_numpy(np.stack([b for _, b, _ in live])).to(dev)
        scores = torch.from_numpy(np.array([s for _, _, s in live], np.float32)).to(dev)
        labels = torch.zeros(len(live), dtype=torch.long, device=dev)
        slot = [SLOTS[t] for t, _, _ in live]
        for t, _, _ in live:
            origin.setdefault(t, np.linalg.inv(pose))
        out = rh.simple_test_scene_step(points, pose, boxes, scores, labels, slot, state)
        # ---- the reference rows, with the existing operators
        m64 = np.stack([origin[t] @ pose for t, _, _ in live])
        m32 = torch.from_numpy(m64[:, :3].reshape(-1, 12).astype(np.float32)).to(dev)
        fixed = rh._boxes_through(boxes, torch.from_numpy(m64[:, :3].reshape(-1, 12)).to(dev))
        for r, (t, box, _) in enumerate(live):     # Tracklet.frame_transform, one box at a time on the host
            trk = Tracklet(torch.from_numpy(box[None].copy()), [0])
            trk.pose_list = [torch.from_numpy(pose)]
            trk.frame_transform(torch.from_numpy(np.linalg.inv(origin[t])))
            assert torch.allclose(trk.boxes[0], fixed[r].cpu(), atol=1e-5, rtol=0), (f, t)
        crop = ctrl_prep.enlarged_boxes(boxes, cfg['extra_width'])
        counts, idx = ctrl_prep.crop_frames_packed(points, [0, len(cloud)], crop, [0, len(live)])
        assert int(counts.max()) <= cfg['max_points']
        row = torch.repeat_interleave(torch.arange(len(live)), counts).to(dev)
        src, m = points[idx], m32[row]
        fma = lambda a, b, c: (a.double() * b.double() + c.double()).float()
        xyz = torch.stack([fma(src[:, 2], m[:, 4 * c + 2], fma(src[:, 1], m[:, 4 * c + 1], fma(src[:, 0], m[:, 4 * c], m[:, 4 * c + 3])))
                           for c in range(3)], 1)
        keep = ((xyz > rng[:3]) & (xyz < rng[3:])).all(1)
        fixed_host = fixed.cpu()
        deco = torch.tensor([[float(b[6]) / 3.1415] + (b[3:6] / 10).tolist() + [float(s)] for b, s in zip(fixed_host, scores.cpu())])
        feats = torch.cat([src[:, 3:5], deco.to(dev)[row]], 1)
        xyz, feats, row = xyz[keep].contiguous(), feats[keep].contiguous(), row[keep]
        # (what the kernel wrote, for the record: equal rows make equal steps)
        k_xyz, k_feats, k_row, k_counts = S.scene_step_rows(points, boxes, scores, transforms=m32, extra_width=cfg['extra_width'],
                                                            point_cloud_range=cfg['point_cloud_range'],
                                                            max_points=cfg['max_points'], deco_boxes=fixed)
        assert torch.equal(k_row, row) and torch.equal(k_counts, out['num_points']) and torch.equal(k_counts, counts)
        err = np.abs(k_xyz.cpu().numpy().astype(np.float64) - R.transform64(src[keep, :3].cpu().numpy(), m32[row].cpu().numpy()))
        assert (err <= R.transform_bound(src[keep, :3].cpu().numpy(), m32[row].cpu().numpy())).all()
        xyz_equal, feats_equal = xyz_equal and torch.equal(k_xyz, xyz), feats_equal and torch.equal(k_feats, feats)
        ref = rh.simple_test_step(xyz, feats, row, fixed, scores, labels, slot, ref_state)
        twins = [rh.simple_test_step(xyz, feats, row, fixed, scores, labels, slot, s) for s in twin_states]
        # ---- the assertions
        assert torch.equal(out['valid'], ref['valid'])
        want_valid = [(t, f - STARTS[t]) != EMPTY for t, _, _ in live]
        assert out['valid'].tolist() == want_valid
        for key in worst:
            scale = float(ref[key].double().abs().max())
            d0[key] = max([d0[key]] + [float((twin[key].double() - ref[key].double()).abs().max()) / scale for twin in twins])
            worst[key] = max(worst[key], float((out[key].double() - ref[key].double()).abs().max()) / scale)
        inv64 = np.linalg.inv(m64)[:, :3].reshape(-1, 12)
        got, refined = out['boxes_ego'].cpu().numpy(), out['boxes'].cpu().numpy()
        for r, ok in enumerate(want_valid):
            if not ok:
                seen_invalid = True
                assert torch.equal(out['boxes_ego'][r], boxes[r]) and int(out['num_points'][r]) == 0
                continue
            centre = R.transform64(refined[r:r + 1, :3], inv64[r])[0]
            assert (np.abs(got[r, :3] - centre) <= R.transform_bound(refined[r:r + 1, :3], inv64[r])[0]).all(), (f, r)
            assert np.array_equal(got[r, 3:6], refined[r, 3:6])
            yaw = refined[r, 6].astype(np.float64)
            hv = inv64[r].reshape(3, 4)[:2, :2] @ np.array([np.sin(yaw), np.cos(yaw)])
            turn = np.arctan2(hv[0], hv[1]) - got[r, 6]
            assert abs((turn + np.pi) % (2 * np.pi) - np.pi) <= 2.0 ** -22, (f, r)       # (an ulp of a yaw below 4)
    assert seen_invalid and state.frames == [FRAMES, 0, FRAMES] and ref_state.frames == state.frames
    assert state.origin[1] is None and np.array_equal(state.origin[2], origin[0]) and np.array_equal(state.origin[0], origin[1])
    print(f'scene step against the existing operators: xyz bit-equal {xyz_equal}, feats bit-equal {feats_equal}; d0 {d0}; '
          f'scene step against reference {worst}')
    for key in worst:
        assert worst[key] <= 2 * d0[key] + 1e-7, (key, worst[key], d0[key])


def test_single_step_refusals_and_empty_call_leave_the_state_alone(dev, model):
    """The single step behaves as the chunked call does (one host body under both): a call without boxes returns the empty
    dict of the chunked call -- its keys, with ``occ=True`` its three more, every value of length 0 -- and launches nothing;
    a step refused after its slot check (a float64 cloud, which scene_step_rows reports; a wrong test_cfg.online_occ, which
    is reported before any launch) leaves origins, frame counters and the K/V cache as they were; a plain step of two
    boxes on the same state then succeeds and sets both origins."""
    rh = model.roi_head
    state = rh.online_begin(2, dev, cap=2)
    boxes = torch.tensor([[10, 0, 0, 2, 4.5, 1.6, 0.1], [10, 10, 0, 2, 4.5, 1.6, -0.2]], device=dev)
    g = np.random.default_rng(8)
    xyz = np.concatenate([boxes.cpu().numpy()[[0, 0, 0, 0, 1, 1, 1, 1], :3] + g.uniform(0.1, 0.6, (8, 3)), g.random((8, 2))], 1)
    points = torch.from_numpy(xyz.astype(np.float32)).to(dev)
    scores, labels, pose = torch.tensor([0.5, 0.6], device=dev), torch.zeros(2, dtype=torch.long, device=dev), ego_pose(1)
    snapshot = lambda: (list(state.frames), list(state.origin), state.cache.pos.clone(), [t.clone() for t in state.cache.k + state.cache.v])

    def unchanged(before):
        now = snapshot()
        return (now[0] == before[0] and now[1] == before[1] == [None, None] and torch.equal(now[2], before[2])
                and all(torch.equal(a, b) for a, b in zip(now[3], before[3])))

    before = snapshot()
    sizes, poses = [8], pose[None]
    for occ in (False, True):                                               # (c)
        want = rh.simple_test_scene_steps(points, sizes, poses, boxes[:0], scores[:0], labels[:0], [], [], state, occ=occ)
        got = rh.simple_test_scene_step(points, pose, boxes[:0], scores[:0], labels[:0], [], state, occ=occ)
        assert set(got) == set(want) and ('occ_ego' in got) == occ and all(len(v) == 0 for v in got.values())
        assert got['boxes_ego'].shape == (0, 7) and unchanged(before)
    with pytest.raises(L.OcoccError, match='float32'):                      # (a)
        rh.simple_test_scene_step(points.double(), pose, boxes[:1], scores[:1], labels[:1], [0], state)
    assert state.origin[0] is None and unchanged(before)
    rh.test_cfg['online_occ'] = dict(chunk=0)                               # (b)
    try:
        with pytest.raises(ValueError, match='online_occ'):
            rh.simple_test_scene_step(points, pose, boxes[:1], scores[:1], labels[:1], [0], state, occ=True)
    finally:
        del rh.test_cfg['online_occ']
    assert state.origin[0] is None and state.frames[0] == 0 and unchanged(before)
    out = rh.simple_test_scene_step(points, pose, boxes, scores, labels, [0, 1], state)
    assert out['num_points'].tolist() == [4, 4] and state.frames == [1, 1]
    assert all(np.array_equal(o, np.linalg.inv(pose)) for o in state.origin)


def test_replay_of_a_synthetic_raw_tree(dev, model, tmp_path):
    """G: make_synthetic_raw's tree (1 segment, 2 objects and one false positive above every point, 6 frames, 500 background
    points) replayed through tools/online_raw.py: one output object per input object with its id and timestamp, finite
    boxes, objects whose box held no point unchanged, every slot released"""
    import importlib.util
    from objectcentricocccompletion_amd import waymo_io
    tools = os.path.join(ROOT, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import make_synthetic_raw
    spec = importlib.util.spec_from_file_location('ococc_tools_online_raw', os.path.join(tools, 'online_raw.py'))
    online_raw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(online_raw)
    root = str(tmp_path / 'raw')
    make_synthetic_raw.main([root, '--segments', '1', '--tracklets', '2', '--frames', '6', '--background', '500'])
    out = str(tmp_path / 'refined.bin')
    records, state = online_raw.replay(model, os.path.join(root, 'synthetic_vehicle.yaml'), slots=4, out=out,
                                       poses=os.path.join(root, 'poses.pkl'))
    assert state.frames == [0, 0, 0, 0] and state.origin == [None] * 4 and state.cache.cap == 6
    src = waymo_io.read_bin(os.path.join(root, 'waymo_format', 'pred.bin'))
    dst = waymo_io.read_bin(out)
    key = lambda o: (o['context_name'], o['id'], o['frame_timestamp_micros'])
    assert len(dst) == len(src) == len(records) and sorted(map(key, dst)) == sorted(map(key, src)) and len(set(map(key, dst))) == len(dst)
    assert all(np.isfinite([o[k] for k in ('center_x', 'center_y', 'center_z', 'width', 'length', 'height', 'heading', 'score')]).all()
               for o in dst)
    tracker = {(t.segment_name, t.id): t for t in waymo_io.generate_tracklets(src)}
    refined = 0
    for r in records:
        t = tracker[(r['segment'], r['id'])]
        i = t.ts2index[r['timestamp']]
        assert np.isfinite(r['box']).all() and r['box'].shape == (7,)
        if r['num_points'] == 0:
            assert not r['refined'] and np.array_equal(r['box'], t.boxes[i].numpy()) and r['score'] == float(t.scores[i])
        refined += r['refined']
    assert sum(r['num_points'] == 0 for r in records) >= 6 and refined >= 6           # the false positive; the two objects
    with pytest.raises(L.OcoccError, match='--slots'):
        online_raw.replay(model, os.path.join(root, 'synthetic_vehicle.yaml'), slots=2, poses=os.path.join(root, 'poses.pkl'))
