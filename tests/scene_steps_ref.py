"""The many-cloud form of csrc/scene_rows.hip for the tests, twice:

``scene_steps``: the numpy restatement, built on scene_rows_ref.scene_rows -- a box sees the points of its own frame only,
the output is in the caller's row order (checked on hand-made cases by test_scene_steps_cpu.py).

``per_frame_rows``: the oracle of the GPU tests -- the existing one-cloud operator scene_rows.scene_step_rows run once per
frame on that frame's cloud and rows, the results put in the caller's row order."""
import numpy as np

import scene_rows_ref as R
from test_gpu_scene_rows import local_to_xy, scene        # noqa: F401 (the synthetic frame of the one-cloud tests)


def scene_steps(points, cloud_sizes, crop_boxes, frame_rows, transforms=None, rng=None, cap=-1, attr_dims=0, row_feats=None):
    """points [N, C]: the clouds back to back, cloud_sizes their lengths; crop_boxes [n, 7], transforms [n, 12], row_feats
    [n, K] in the caller's row order, frame_rows [n] the cloud of each row -> what R.scene_rows returns, row = the caller's
    row, sorted by (row, point index within the frame)."""
    points, crop_boxes = np.asarray(points, R.F), np.asarray(crop_boxes, R.F).reshape(-1, 7)
    offs = np.concatenate([[0], np.cumsum(cloud_sizes)]).astype(np.int64)
    assert offs[-1] == len(points) and len(frame_rows) == len(crop_boxes)
    K = 0 if row_feats is None else np.asarray(row_feats).shape[1]
    xyz, feats, row, counts = [], [], [], np.zeros(len(crop_boxes), np.int64)
    for i, f in enumerate(frame_rows):
        one = R.scene_rows(points[offs[f]:offs[f + 1]], crop_boxes[i:i + 1], None if transforms is None else np.asarray(transforms)[i:i + 1],
                           rng, cap, attr_dims, None if row_feats is None else np.asarray(row_feats)[i:i + 1])
        xyz.append(one[0]), feats.append(one[1]), row.append(one[2] + i)
        counts[i] = one[3][0]
    cat = lambda parts, shape: np.concatenate(parts, 0) if parts else np.zeros(shape)
    return cat(xyz, (0, 3)), cat(feats, (0, attr_dims + K)).astype(R.F), cat(row, (0,)).astype(np.int64), counts


def per_frame_rows(points, cloud_sizes, boxes, scores, frame_rows, transforms=None, deco_boxes=None, max_points=-1, **kw):
    """scene_rows.scene_step_rows once per frame (device tensors; frame_rows and cloud_sizes on the host) -> (xyz, feats,
    row, counts) in the caller's row order, as scene_steps_rows returns them"""
    import torch
    from objectcentricocccompletion_amd import scene_rows as S
    dev, n = points.device, len(frame_rows)
    offs = [0] + np.cumsum(cloud_sizes).tolist()
    counts = torch.zeros((n,), dtype=torch.int64)
    pieces = {}
    for f in range(len(cloud_sizes)):
        rows = [i for i, v in enumerate(frame_rows) if v == f]
        if not rows:
            continue
        idx = torch.tensor(rows, device=dev)
        pick = lambda t: None if t is None else t[idx].contiguous()
        xyz, feats, row, c = S.scene_step_rows(points[offs[f]:offs[f + 1]], boxes[idx].contiguous(), scores[idx], transforms=pick(transforms),
                                               deco_boxes=pick(deco_boxes), max_points=max_points, **kw)
        kept = (c.clamp(max=max_points) if max_points > 0 else c).tolist()
        assert row.tolist() == [j for j, k in enumerate(kept) for _ in range(k)]
        for i, cnt, x, ft in zip(rows, c.tolist(), torch.split(xyz, kept), torch.split(feats, kept)):
            counts[i], pieces[i] = cnt, (x, ft)
    width = kw.get('attr_dims', 2) + S.ROW_FEAT_DIM
    xs = [pieces[i][0] for i in range(n) if i in pieces] or [torch.zeros((0, 3), device=dev)]
    fs = [pieces[i][1] for i in range(n) if i in pieces] or [torch.zeros((0, width), device=dev)]
    lens = torch.tensor([pieces[i][0].size(0) if i in pieces else 0 for i in range(n)], dtype=torch.int64)
    return torch.cat(xs), torch.cat(fs), torch.repeat_interleave(torch.arange(n), lens).to(dev), counts
