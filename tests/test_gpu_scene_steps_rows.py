"""The scene clouds of several sensor frames into step rows in one call, on the MI355X (csrc/scene_rows.hip with
blockIdx.y = frame: ococc_scene_rows_frames_count / _fill, scene_rows.scene_steps_rows).

The oracle is the existing one-cloud operator, scene_rows.scene_step_rows, run once per frame on that frame's cloud and
rows, its results put in the caller's row order (scene_steps_ref.per_frame_rows).  Everything is compared with
torch.equal: xyz, feats, row and counts.  Shapes: the smallest that reach the edges of the wave tile (1024 points), the
workgroup tile (4096 points) and the LDS chunk (64 boxes)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_rows_ref as R        # noqa: E402
import scene_steps_ref as RS      # noqa: E402
from objectcentricocccompletion_amd import _lib as L        # noqa: E402
from objectcentricocccompletion_amd import ctrl_prep        # noqa: E402
from objectcentricocccompletion_amd import scene_rows as S  # noqa: E402

pytestmark = pytest.mark.gpu
PAD = 3            # rows behind M in the output buffers of raw_frames: must stay as they were filled
RANGE = [-204.7, -204.7, -3.99, 204.7, 204.7, 7.99]


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


def rigid(g, n, shift=80.0):
    """n row-major 3x4 matrices [n, 12] f32: a rotation about an oblique axis and a translation of up to ``shift`` m"""
    mats = np.zeros((n, 3, 4))
    for b in range(n):
        q, _ = np.linalg.qr(g.normal(size=(3, 3)))
        mats[b, :, :3], mats[b, :, 3] = q, g.uniform(-shift, shift, 3)
    return mats.reshape(n, 12).astype(np.float32)


def ego_moves(g, n):
    """n matrices [n, 12] f32 as ego motion makes them: a turn about z, up to 215 m along x and y (some rows end up across
    a face of RANGE, whose x and y faces are at 204.7 m), up to 1 m along z (none leaves RANGE in z)"""
    mats = np.zeros((n, 3, 4))
    a = g.uniform(-np.pi, np.pi, n)
    mats[:, 0, 0], mats[:, 0, 1], mats[:, 1, 0], mats[:, 1, 1], mats[:, 2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a), 1
    mats[:, :2, 3], mats[:, 2, 3] = g.uniform(-215, 215, (n, 2)), g.uniform(-1, 1, n)
    return mats.reshape(n, 12).astype(np.float32)


def assert_equal(got, want, what):
    for g, w, name in zip(got, want, ('xyz', 'feats', 'row', 'counts')):
        assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w), (what, name)
    assert not got[3].is_cuda


def many_frames(dev, sizes, boxes_per_frame, C, seed):
    """clouds and boxes of RS.scene per frame, the rows of all frames in a random (not frame-major) caller's order"""
    g = np.random.default_rng(seed)
    clouds, boxes, frame_rows = [], [], []
    for f, (N, n) in enumerate(zip(sizes, boxes_per_frame)):
        pts, bx = RS.scene(N, n, C, seed=seed + 17 * f)
        clouds.append(pts)
        boxes.append(bx)
        frame_rows += [f] * n
    order = g.permutation(len(frame_rows))
    boxes, frame_rows = np.concatenate(boxes)[order], [frame_rows[i] for i in order]
    points = torch.from_numpy(np.concatenate(clouds)).to(dev)
    scores = torch.from_numpy(g.random(len(frame_rows)).astype(np.float32)).to(dev)
    return points, torch.from_numpy(boxes).to(dev), scores, frame_rows


def test_tile_and_chunk_edges_in_one_call(dev):
    """1: clouds of 0, 1, 1023, 1024, 1025 and 4097 points in one call; 3 boxes on most frames, none on one, 65 on one;
    the caller's rows in a shuffled order.  Plain, and with per-row transforms, the range and a cap.  Then the same call
    behind 520 empty clouds: with that many frames the launch no longer splits a frame's boxes, so the workgroups of the
    65-box frame walk a second LDS chunk."""
    sizes, per_frame = [0, 1, 1023, 1024, 1025, 4097], [3, 3, 0, 65, 3, 3]
    points, boxes, scores, frame_rows = many_frames(dev, sizes, per_frame, 5, seed=100)
    n = len(frame_rows)
    assert frame_rows != sorted(frame_rows)
    m32 = torch.from_numpy(ego_moves(np.random.default_rng(1), n)).to(dev)
    for kw in (dict(extra_width=0.25), dict(extra_width=0.25, transforms=m32, point_cloud_range=RANGE, max_points=7)):
        want = RS.per_frame_rows(points, sizes, boxes, scores, frame_rows, **kw)
        if 'transforms' in kw:     # the range cuts some rows and leaves most
            assert 0 < int(want[3].sum()) < plain_total
        plain_total = int(want[3].sum())
        assert int(want[3].sum()) > 500 and int((want[3] == 0).sum()) >= 4 and int(want[3].max()) > 7
        assert_equal(S.scene_steps_rows(points, sizes, boxes, scores, frame_rows, **kw), want, sorted(kw))
        pad = 520
        late = S.scene_steps_rows(points, [0] * pad + sizes, boxes, scores, [f + pad for f in frame_rows], **kw)
        assert_equal(late, want, ('behind empty clouds', sorted(kw)))


def test_same_box_in_two_frames(dev):
    """2: one box given for two frames whose clouds differ: each row holds the points of its own frame only"""
    g = np.random.default_rng(2)
    box = np.array([[3, 2, 0, 2, 4.5, 1.6, 0.4]], np.float32)

    def cloud(inside, outside, tag):
        dx, dy = RS.local_to_xy(box[0], (g.random(inside) - 0.5) * 4.0, (g.random(inside) - 0.5) * 1.6)
        xyz = np.concatenate([np.stack([3 + dx, 2 + dy, 0.1 + 1.4 * g.random(inside)], 1),
                              np.concatenate([g.uniform(30, 60, (outside, 2)), g.uniform(0, 2, (outside, 1))], 1)])
        xyz = xyz[g.permutation(len(xyz))]
        return np.concatenate([xyz, np.full((len(xyz), 1), tag), np.arange(len(xyz))[:, None]], 1).astype(np.float32)   # tag, place in the cloud

    a, b = cloud(40, 200, 1.0), cloud(55, 150, 2.0)
    points = torch.from_numpy(np.concatenate([a, b])).to(dev)
    boxes = torch.from_numpy(np.repeat(box, 2, 0)).to(dev)
    scores = torch.tensor([0.5, 0.7], device=dev)
    for frame_rows, tags in (([0, 1], [1.0, 2.0]), ([1, 0], [2.0, 1.0])):
        xyz, feats, row, counts = S.scene_steps_rows(points, [len(a), len(b)], boxes, scores, frame_rows, extra_width=0.0)
        assert counts.tolist() == [40 if t == 1.0 else 55 for t in tags]
        for r, t in enumerate(tags):
            mine = feats[row == r]
            assert bool((mine[:, 0] == t).all()) and bool((mine[1:, 1] > mine[:-1, 1]).all())    # its frame's, in cloud order
        assert_equal((xyz, feats, row, counts),
                     RS.per_frame_rows(points, [len(a), len(b)], boxes, scores, frame_rows, extra_width=0.0), frame_rows)


def test_transforms_range_overlap_and_nan(dev):
    """3: frame 0 -- overlapping boxes (a point in two rows of one frame), a different rigid matrix per row, NaN and
    infinite coordinates: the written xyz within R.transform_bound of the float64 transform of the untransformed rows.
    Frame 1 -- the range faces of the one-cloud range test under identity matrices: a written coordinate exactly on a face
    is outside, its neighbour inside is a row; a NaN z passes the box and is dropped by the range; a NaN x is in no box."""
    f = np.float32
    hi, lo = f(204.7), f(-3.99)
    face_box = np.array([[204, 0, -5, 4, 4, 4, 0.0], [0, 0, -5, 4, 4, 4, 0.3]], f)
    face_pts = np.array([[hi, 0, -2, 1], [np.nextafter(hi, f(0)), 0, -2, 2], [np.nextafter(hi, f(999)), 0, -2, 3],
                         [0, 0, lo, 4], [0, 0, np.nextafter(lo, f(0)), 5], [0, 0, np.nextafter(lo, f(-9)), 6],
                         [0.5, 0.5, -2, 7], [0, 0, np.nan, 8], [np.nan, 0, -2, 9]], f)
    pts, bx = RS.scene(3000, 12, 4, seed=31)
    points = torch.from_numpy(np.concatenate([pts, face_pts])).to(dev)
    sizes = [len(pts), len(face_pts)]
    # caller's rows: face box 1, the 12 boxes of frame 0, face box 0
    boxes = torch.from_numpy(np.concatenate([face_box[1:], bx, face_box[:1]])).to(dev)
    frame_rows = [1] + [0] * 12 + [1]
    scores = torch.linspace(0.1, 0.9, 14, device=dev)
    ident = np.eye(4, dtype=f)[:3].reshape(1, 12)
    m32 = torch.from_numpy(np.concatenate([ident, rigid(np.random.default_rng(32), 12), ident])).to(dev)
    kw = dict(extra_width=0.0, attr_dims=1)
    plain = S.scene_steps_rows(points, sizes, boxes, scores, frame_rows, **kw)
    assert plain[3][0] == 5 and plain[3][13] == 3                       # (a NaN z passes the box test, a NaN x does not)
    got = S.scene_steps_rows(points, sizes, boxes, scores, frame_rows, transforms=m32, point_cloud_range=RANGE, **kw)
    assert_equal(got, RS.per_frame_rows(points, sizes, boxes, scores, frame_rows, transforms=m32, point_cloud_range=RANGE, **kw),
                 'transforms and range')
    xyz, feats, row, counts = got
    assert counts.tolist()[0] == 2 and counts.tolist()[13] == 1
    assert feats[row == 0][:, 0].tolist() == [5, 7] and feats[row == 13][:, 0].tolist() == [2]
    assert torch.equal(xyz[row == 0], points[len(pts) + torch.tensor([4, 6], device=dev), :3])
    assert torch.equal(xyz[row == 13], points[len(pts) + 1:len(pts) + 2, :3])
    # frame 0 without the range: the plain rows, moved
    xyz, feats, row, counts = S.scene_steps_rows(points, sizes, boxes, scores, frame_rows, transforms=m32, **kw)
    assert torch.equal(counts, plain[3])
    mid = (row >= 1) & (row <= 12)
    pmid = (plain[2] >= 1) & (plain[2] <= 12)
    assert torch.equal(row[mid], plain[2][pmid]) and torch.equal(feats[mid], plain[1][pmid])
    src, rows = plain[0][pmid].cpu().numpy(), plain[2][pmid].cpu().numpy()
    assert (np.unique(src, axis=0, return_counts=True)[1] >= 2).sum() > 5, 'no point lies in two boxes'
    m_rows = m32.cpu().numpy().astype(np.float64)[rows]
    err = np.abs(xyz[mid].cpu().numpy().astype(np.float64) - R.transform64(src, m_rows))
    bound = R.transform_bound(src, m_rows)
    print(f'transform: {len(src)} rows, largest error / bound {float((err / bound).max()):.3f}')
    assert (err <= bound).all()


@pytest.mark.parametrize('cap', [1, 5, 64])
def test_cap_is_the_even_pick_per_frame(dev, cap):
    """4: boxes with m = cap, cap + 1 and 2 cap + 1 members in three different frames (and one box over all three): the
    capped rows are S.even_pick of the uncapped rows, counts stay uncapped"""
    g = np.random.default_rng(40 + cap)
    ms = [cap, cap + 1, 2 * cap + 1]
    box = np.array([[5, -3, 0, 2, 4.5, 1.6, 0.9]], np.float32)
    clouds = []
    for m in ms:
        dx, dy = RS.local_to_xy(box[0], (g.random(m) - 0.5) * 4.0, (g.random(m) - 0.5) * 1.6)
        xyz = np.concatenate([np.stack([5 + dx, -3 + dy, 0.1 + 1.4 * g.random(m)], 1),
                              np.concatenate([g.uniform(-60, -30, (100, 2)), g.uniform(0, 2, (100, 1))], 1)])
        clouds.append(np.concatenate([xyz, np.arange(len(xyz))[:, None]], 1)[g.permutation(len(xyz))].astype(np.float32))
    points = torch.from_numpy(np.concatenate(clouds)).to(dev)
    sizes, frame_rows = [len(c) for c in clouds], [2, 0, 1]
    boxes, scores = torch.from_numpy(np.repeat(box, 3, 0)).to(dev), torch.tensor([0.2, 0.4, 0.6], device=dev)
    kw = dict(extra_width=0.0, attr_dims=1)
    full = S.scene_steps_rows(points, sizes, boxes, scores, frame_rows, **kw)
    got = S.scene_steps_rows(points, sizes, boxes, scores, frame_rows, max_points=cap, **kw)
    want_counts = [ms[f] for f in frame_rows]
    assert full[3].tolist() == want_counts and got[3].tolist() == want_counts
    first = np.concatenate([[0], np.cumsum(want_counts)])
    keep = torch.tensor([first[r] + j for r, m in enumerate(want_counts) for j, _ in S.even_pick(m, cap)], dtype=torch.long,
                        device=dev)
    assert len(keep) == 3 * cap == got[0].size(0)
    for a, b in zip(got[:3], full[:3]):
        assert torch.equal(a, b[keep])
    assert_equal(got, RS.per_frame_rows(points, sizes, boxes, scores, frame_rows, max_points=cap, **kw), cap)


def test_one_frame_is_the_one_cloud_operator(dev):
    """5: F = 1 equals scene_step_rows bit for bit -- 9000 points (three workgroups along the points), 70 boxes"""
    pts, bx = RS.scene(9000, 70, 6, seed=21)
    points, boxes = torch.from_numpy(pts).to(dev), torch.from_numpy(bx).to(dev)
    scores = torch.linspace(0.1, 0.9, 70, device=dev)
    m32 = torch.from_numpy(ego_moves(np.random.default_rng(5), 70)).to(dev)
    for kw in (dict(extra_width=0.25), dict(extra_width=0.25, transforms=m32, point_cloud_range=RANGE, max_points=9)):
        want = S.scene_step_rows(points, boxes, scores, **kw)
        assert int(want[3].sum()) > 1000
        assert_equal(S.scene_steps_rows(points, [9000], boxes, scores, [0] * 70, **kw), want, sorted(kw))


def raw_frames(points, sizes, crop, frame_rows, ws, A=0, cap=-1):
    """the two exports called as scene_steps_rows calls them, on the caller's workspace; the outputs are PAD rows longer
    than M, filled with a sentinel that must survive"""
    dev = points.device
    F, n, N = len(sizes), crop.size(0), points.size(0)
    order, box_offsets = S.frame_major(frame_rows, F)
    cloud_offsets = [0] + np.cumsum(sizes).tolist()
    plan = torch.tensor(cloud_offsets + box_offsets + order, dtype=torch.int64).to(dev)
    order_dev = plan[2 * F + 2:]
    crop_f = crop[order_dev].contiguous()
    max_pts, max_boxes = max(sizes), max(box_offsets[f + 1] - box_offsets[f] for f in range(F))
    assert ws.numel() >= int(L.lib.ococc_scene_rows_workspace_bytes(max_pts, n))
    counts = torch.full((n,), -7, dtype=torch.int64, device=dev)
    head = (L.ptr(points), N, points.size(1), L.ptr(plan[:F + 1]), L.ptr(crop_f), n, L.ptr(plan[F + 1:2 * F + 2]), F, max_pts,
            max_boxes, None, None)
    L.check(L.lib.ococc_scene_rows_frames_count(*head, L.ptr(counts), L.ptr(ws), ws.numel(), L.stream()), 'count')
    totals = counts.cpu()
    oh = torch.tensor(order, dtype=torch.int64)
    caller = torch.zeros(n, dtype=torch.int64)
    caller[oh] = totals
    kept = caller.clamp(max=cap) if cap > 0 else caller
    ends = torch.cumsum(kept, 0)
    M = int(ends[-1])
    sd = torch.stack([totals, (ends - kept)[oh]]).to(dev)
    xyz = torch.full((M + PAD, 3), -777.0, device=dev)
    feats = torch.full((M + PAD, A), -777.0, device=dev)
    row = torch.full((M + PAD,), -777, dtype=torch.int64, device=dev)
    L.check(L.lib.ococc_scene_rows_frames_fill(*head, A, None, 0, L.ptr(order_dev), cap, L.ptr(sd[0]), L.ptr(sd[1]), M, L.ptr(xyz),
                                               L.ptr(feats), L.ptr(row), L.ptr(ws), ws.numel(), L.stream()), 'fill')
    assert bool((xyz[M:] == -777).all()) and bool((feats[M:] == -777).all()) and bool((row[M:] == -777).all())
    return xyz[:M], feats[:M], row[:M], caller


def crop_rows_per_frame(points, sizes, crop, frame_rows, A):
    """the same rows from the existing offline crop (ctrl_prep.crop_frames_packed), per frame, in the caller's order"""
    dev = points.device
    offs = [0] + np.cumsum(sizes).tolist()
    parts, counts = {}, torch.zeros(len(frame_rows), dtype=torch.int64)
    for f in range(len(sizes)):
        rows = [i for i, v in enumerate(frame_rows) if v == f]
        if not rows:
            continue
        cloud = points[offs[f]:offs[f + 1]]
        c, idx = ctrl_prep.crop_frames_packed(cloud, [0, cloud.size(0)], crop[torch.tensor(rows, device=dev)].contiguous(), [0, len(rows)])
        for i, piece in zip(rows, torch.split(idx, c.tolist())):
            parts[i], counts[i] = cloud[piece], len(piece)
    rows = [parts[i] for i in range(len(frame_rows)) if i in parts] or [points[:0]]
    allp = torch.cat(rows)
    return allp[:, :3], allp[:, 3:3 + A], torch.repeat_interleave(torch.arange(len(frame_rows)), counts).to(dev), counts


def test_empty_calls_and_stale_workspace(dev):
    """6: n = 0; all clouds empty; no point in any box; and a small call after a large one on ONE workspace (the large
    call's per-tile counts stay behind it), each against the existing offline crop, nothing written behind row M"""
    pts, bx = RS.scene(3000, 5, 5, seed=61)
    points, boxes = torch.from_numpy(pts).to(dev), torch.from_numpy(bx).to(dev)
    scores = torch.ones(5, device=dev)
    none = S.scene_steps_rows(points, [1000, 2000], boxes[:0], scores[:0], [])
    assert none[0].shape == (0, 3) and none[1].shape == (0, 7) and none[2].shape == (0,) and none[3].shape == (0,)
    none = S.scene_steps_rows(points[:0], [0, 0, 0], boxes, scores, [2, 0, 1, 1, 0])
    assert none[0].shape == (0, 3) and none[1].shape == (0, 7) and none[2].dtype == torch.int64 and none[3].tolist() == [0] * 5
    far = boxes.clone()
    far[:, :2] += 900
    none = S.scene_steps_rows(points, [1000, 2000], far, scores, [1, 0, 1, 0, 1], point_cloud_range=RANGE, max_points=4)
    assert none[0].shape == (0, 3) and none[1].shape == (0, 7) and none[3].tolist() == [0] * 5 and not none[3].is_cuda
    ws = torch.empty((int(L.lib.ococc_scene_rows_workspace_bytes(4500, 73)),), dtype=torch.uint8, device=dev)
    for sizes, per_frame, seed in (([4500, 4100], [70, 3], 62), ([700, 1500, 0], [4, 0, 5], 63), ([4500, 4100], [70, 3], 62)):
        points, boxes, _, frame_rows = many_frames(dev, sizes, per_frame, 5, seed)
        crop = ctrl_prep.enlarged_boxes(boxes, 0.25)
        got, want = raw_frames(points, sizes, crop, frame_rows, ws, A=2), crop_rows_per_frame(points, sizes, crop, frame_rows, 2)
        assert int(want[3].sum()) > 0
        assert_equal(got, want, sizes)
