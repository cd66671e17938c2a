"""occ_ops.occ_merge_frames (the frames exports of csrc/occ_merge.hip) on the MI355X against its numpy restatement
tests/occ_merge_frames_ref.py: the bytes of the whole output, the segment offsets and the survivors per row; the operator
chain occ_merge_frames_aten and a second run give the same bytes; every segment is what occ_ops.occ_merge returns for
that frame alone.  The cases: one frame, rows interleaved over three frames (a real permutation, a row of one tile, a row of
more than a block of tiles, empty rows), frames without a row (first, middle, last), without a cell, with an empty cloud,
R = 0, F = 0, N = 0, cloud seams inside a wave, inside a copy block and on a copy-block edge, a frame where nothing survives
between frames where cells do, everything and nothing surviving, row_score against column 3, scores at and next to the
threshold, NaN / inf / -0.0 / denormal scores, flags with drop_observed on and off, every use_dim form.  And the table check
on the device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_merge_frames_ref as ref                                            # noqa: E402

pytestmark = pytest.mark.gpu
CASES = ref.cases()


def _device(c, dev):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(points=t(c['points']), cloud_sizes=c['cloud_sizes'], occ=t(c['occ']), counts=c['counts'],
                frame_rows=c['frame_rows'], use_dim=c['use_dim'], row_score=t(c['row_score']), flags=t(c['flags']),
                drop_observed=c['drop_observed'], score_threshold=c['score_threshold'])


def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_frames_equal_the_restatement(c, dev):
    from objectcentricocccompletion_amd.occ import occ_ops
    want, want_offsets, want_kept = ref.occ_merge_frames_ref(*ref.args_of(c))
    args = _device(c, dev)
    got, offsets, kept = occ_ops.occ_merge_frames(**args)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_contiguous()
    assert isinstance(offsets, list) and offsets == want_offsets
    assert isinstance(kept, list) and kept == want_kept
    assert _bytes(got) == want.tobytes()
    chain, chain_offsets, chain_kept = occ_ops.occ_merge_frames_aten(**args)
    assert chain_offsets == want_offsets and chain_kept == want_kept and _bytes(chain) == want.tobytes()
    again, _, _ = occ_ops.occ_merge_frames(**args)
    assert _bytes(again) == _bytes(got)
    # every segment is occ_merge on that frame alone
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for f in range(len(c['cloud_sizes'])):
        cloud, cells, cnt, score, flags, rows = ref.frame_parts(f, c['points'], c['cloud_sizes'], c['occ'], c['counts'],
                                                                c['frame_rows'], c['row_score'], c['flags'])
        alone, alone_kept = occ_ops.occ_merge(t(cloud), t(cells), cnt, c['use_dim'], t(score), t(flags), c['drop_observed'],
                                              c['score_threshold'])
        assert _bytes(got[offsets[f]:offsets[f + 1]]) == _bytes(alone), f
        assert [kept[i] for i in rows] == alone_kept, f


def test_one_frame_is_occ_merge(dev):
    from objectcentricocccompletion_amd.occ import occ_ops
    import occ_merge_ref as one
    for c in one.cases():
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        args = (t(c['occ']), c['counts'])
        kw = dict(use_dim=c['use_dim'], row_score=t(c['row_score']), flags=t(c['flags']), drop_observed=c['drop_observed'],
                  score_threshold=c['score_threshold'])
        want, want_kept = occ_ops.occ_merge(t(c['points']), *args, **kw)
        got, offsets, kept = occ_ops.occ_merge_frames(t(c['points']), [len(c['points'])], *args, [0] * len(c['counts']), **kw)
        assert _bytes(got) == _bytes(want) and got.shape == want.shape, c['name']
        assert offsets == [0, want.size(0)] and kept == want_kept, c['name']


def test_table_check_on_the_device(dev, monkeypatch):
    """a frame table that decreases along the order: the export's one-wave check sets row_counts = -1, no tile runs, and
    the operator reports it after its one read-back -- an argument error, nothing is written"""
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd import scene_rows
    from objectcentricocccompletion_amd.occ import occ_ops
    c = next(c for c in CASES if c['name'] == 'interleaved')
    args = _device(c, dev)
    lib = L.lib
    R, M, N, F = len(c['counts']), len(c['occ']), len(c['points']), len(c['cloud_sizes'])
    tiles = int(lib.ococc_occ_select_max_tiles(M, R))
    start = np.cumsum([0] + c['counts'])
    cloud_start = np.cumsum([0] + c['cloud_sizes'])
    order, first = scene_rows.frame_major(c['frame_rows'], F)

    def count(start=start, order=order, frames=c['frame_rows'], cloud_start=cloud_start, first=first):
        up = lambda v: torch.tensor(np.asarray(v), dtype=torch.int64, device=dev)
        tile_start = torch.full((R + 1,), 7, dtype=torch.int64, device=dev)
        tile_counts = torch.full((tiles,), 7, dtype=torch.int32, device=dev)
        row_counts = torch.full((R,), 7, dtype=torch.int64, device=dev)
        tabs = [up(start), up(order), up(frames), up(cloud_start), up(first)]
        L.check(lib.ococc_occ_merge_frames_count(
            L.ptr(args['occ']), M, L.ptr(tabs[0]), L.ptr(tabs[1]), L.ptr(tabs[2]), R, L.ptr(tabs[3]), L.ptr(tabs[4]), F, N, None,
            None, 0, float(c['score_threshold']), L.ptr(tile_start), L.ptr(tile_counts), tiles, L.ptr(row_counts), L.stream()),
            'occ_merge_frames_count')
        return tile_start.tolist(), tile_counts.tolist(), row_counts.tolist()

    want = ref.occ_merge_frames_ref(*ref.args_of(c))[2]
    tile_start, tile_counts, row_counts = count()
    assert row_counts == want and sum(tile_counts) == sum(want)
    assert tile_start == np.cumsum([0] + [-(-c['counts'][r] // 1024) for r in order]).tolist()
    refused = ([0] * (R + 1), [0] * tiles, [-1] * R)
    assert count(order=order[::-1]) == refused                               # the frames decrease along the order
    assert count(order=list(range(R))) == refused                            # the caller's order is not frame-major
    assert count(order=[R] + order[1:]) == refused and count(order=[-1] + order[1:]) == refused
    assert count(frames=[F] + c['frame_rows'][1:]) == refused and count(frames=[-1] + c['frame_rows'][1:]) == refused
    assert count(cloud_start=cloud_start + 1) == refused and count(cloud_start=cloud_start[::-1].copy()) == refused
    assert count(cloud_start=np.concatenate([cloud_start[:-1], [N - 1]])) == refused
    assert count(first=[0, 1, 4, R]) == refused and count(first=[0, 2, 5, R - 1]) == refused
    assert count(start=np.concatenate([start[:-1], [M + 1]])) == refused
    # through the operator: the host's order replaced by one along which the frames decrease
    real = scene_rows.frame_major
    monkeypatch.setattr(scene_rows, 'frame_major', lambda rows, frames: (real(rows, frames)[0][::-1], real(rows, frames)[1]))
    with pytest.raises(L.OcoccError, match='non-decreasing along the order'):
        occ_ops.occ_merge_frames(**args)
    monkeypatch.undo()
    got, _, kept = occ_ops.occ_merge_frames(**args)
    assert kept == want and _bytes(got) == ref.occ_merge_frames_ref(*ref.args_of(c))[0].tobytes()


def test_operator_refuses_on_the_device(dev):
    """the refusals that need device tensors to get past the CPU check"""
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ import occ_ops
    pts, occ = torch.zeros(4, 6, device=dev), torch.zeros(5, 4, device=dev)
    with pytest.raises(L.OcoccError, match='use_dim'):
        occ_ops.occ_merge_frames(pts, [4], occ, [5], [0], use_dim=(0, 1, 6))
    with pytest.raises(L.OcoccError, match='cloud_sizes'):
        occ_ops.occ_merge_frames(pts, [1, 2], occ, [5], [0])
    with pytest.raises(L.OcoccError, match='frame_rows'):
        occ_ops.occ_merge_frames(pts, [1, 3], occ, [2, 3], [0, 2])
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        occ_ops.occ_merge_frames(pts, [1, 3], occ, [2, 3], [1, 0], flags=torch.zeros(5, dtype=torch.uint8), drop_observed=True)
