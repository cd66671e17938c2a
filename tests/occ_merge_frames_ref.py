"""The occupancy-enhanced clouds of several frames in one call (occ_ops.occ_merge_frames, the frames exports of
csrc/occ_merge.hip) restated in plain numpy: occ_merge_ref of tests/occ_merge_ref.py per frame, on the frame's cloud and
the cells, scores and flags of the frame's rows, concatenated.  Also the cases tests/test_gpu_occ_merge_frames.py runs.
No device, no package import."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_merge_ref as one                                                    # noqa: E402

F32 = np.float32
COPY_BLOCK = 2048            # output elements of the real rows per block of the fill kernel


def frame_parts(f, points, cloud_sizes, occ, counts, frame_rows, row_score=None, flags=None):
    """what frame f brings: (its cloud, the cells of its rows, their counts, scores and flags, the rows' indices)"""
    points, occ = np.asarray(points, F32), np.asarray(occ, F32).reshape(-1, 4)
    cloud, cell = np.cumsum([0] + [int(s) for s in cloud_sizes]), np.cumsum([0] + [int(c) for c in counts])
    rows = [i for i, fr in enumerate(frame_rows) if int(fr) == f]
    pick = lambda a: None if a is None else np.concatenate([np.asarray(a)[cell[i]:cell[i + 1]] for i in rows] + [np.asarray(a)[:0]])
    score = None if row_score is None else np.asarray(row_score, F32)[rows]
    return points[cloud[f]:cloud[f + 1]], pick(occ), [int(counts[i]) for i in rows], score, pick(flags), rows


def occ_merge_frames_ref(points, cloud_sizes, occ, counts, frame_rows, use_dim=(0, 1, 2, 3, 4), row_score=None, flags=None,
                         drop_observed=False, score_threshold=0.0):
    """(merged [N + K, D + 2] f32, offsets [F + 1] as a list, survivors per input row as a list): segment f is
    occ_merge_ref of cloud f and the cells of the rows with frame_rows[i] == f, in ascending i"""
    assert len(frame_rows) == len(counts) and sum(int(s) for s in cloud_sizes) == len(points)
    assert all(0 <= int(f) < len(cloud_sizes) for f in frame_rows)
    parts, offsets, kept = [], [0], [0] * len(counts)
    for f in range(len(cloud_sizes)):
        cloud, cells, cnt, score, flg, rows = frame_parts(f, points, cloud_sizes, occ, counts, frame_rows, row_score, flags)
        merged, k = one.occ_merge_ref(cloud, cells, cnt, use_dim, score, flg, drop_observed, score_threshold)
        parts.append(merged)
        offsets.append(offsets[-1] + len(merged))
        for i, v in zip(rows, k):
            kept[i] = int(v)
    width = len(one.use_dim_list(use_dim)) + 2
    merged = np.concatenate(parts + [np.zeros((0, width), F32)], axis=0).astype(F32, copy=False)
    return merged, offsets, kept


def case(name, cloud_sizes, counts, frame_rows, **kw):
    c = one.case(name, int(sum(cloud_sizes)), counts, **kw)
    c.update(cloud_sizes=list(cloud_sizes), frame_rows=list(frame_rows))
    return c


INTERLEAVED = [0, 1, 2, 0, 2, 1, 1]     # with one.STRADDLE: frame 0 rows without a cell; frame 1 one tile exactly, a short
                                        # row and an empty one; frame 2 a row of five tiles (more than a block) and two tiles
SEAMS = [63, 1, 0, 293, 3001]           # at D = 5 (W = 7): seams inside a wave and inside a copy block, a short last block


def cases():
    out = [case('F1', [65], one.STRADDLE, [0] * 7, seed=7)]
    out.append(case('interleaved', [65, 130, 40], one.STRADDLE, INTERLEAVED, seed=1))
    out.append(case('interleaved_row_score', [65, 130, 40], one.STRADDLE, INTERLEAVED, seed=2,
                    row_score=np.array([0.9, 0.3, 0.1, 0.9, 0.4, 0.2, 0.9], F32)))
    out.append(case('no_row_first', [10, 65, 30], [700, 1100, 40], [1, 2, 1], seed=3))
    out.append(case('no_row_middle', [10, 65, 30], [700, 1100, 40], [0, 2, 0], seed=4))
    out.append(case('no_row_last', [10, 65, 30], [700, 1100, 40], [0, 1, 0], seed=5))
    out.append(case('no_cell_frame', [10, 65, 30], [700, 0, 1100, 0], [0, 1, 2, 1], seed=6))
    out.append(case('empty_cloud', [65, 0, 30], [700, 1100, 40], [2, 1, 0], seed=8))
    out.append(case('R0_F3', [5, 0, 70], [], []))
    out.append(case('F0', [], [], []))
    out.append(case('N0_cells', [0, 0], [40, 1030], [1, 0], seed=9))
    out.append(case('seams', SEAMS, [40, 25, 33, 1030, 17], [4, 0, 3, 1, 2], seed=10))
    out.append(case('seams_no_cells', SEAMS, [0, 0], [1, 3]))
    # 2048 rows of W = 7 are seven whole copy blocks: the seam between the clouds is a block edge
    out.append(case('seam_on_block_edge', [COPY_BLOCK, 100], [300, 1100], [1, 0], seed=11))
    out.append(case('dead_middle_frame', [65, 33, 70], [300, 1100, 50, 20, 1500], [0, 1, 2, 1, 0], seed=12,
                    row_score=np.array([0.9, 0.1, 0.9, 0.1, 0.9], F32)))
    out.append(case('all_survive', [65, 130, 40], one.STRADDLE, INTERLEAVED, threshold=-np.inf, seed=13))
    out.append(case('none_survive', [65, 130, 40], one.STRADDLE, INTERLEAVED, threshold=np.inf, seed=14))
    for thr in (0.25, 0.0):
        sc = one.edge_scores(thr)
        cells = np.random.default_rng(5).normal(0, 5, (len(sc), 4)).astype(F32)
        cells[:, 3] = sc
        out.append(case(f'edges_col3_{thr}', [7, 3], [3, 0, len(sc) - 3], [1, 0, 0], threshold=thr, occ=cells))
        out.append(case(f'edges_row_score_{thr}', [7, 3, 5], [2] * len(sc), [i % 3 for i in range(len(sc))], threshold=thr,
                        row_score=sc, seed=3))
    for drop in (False, True):
        out.append(case(f'flags_drop{int(drop)}', [65, 130, 40], one.STRADDLE, INTERLEAVED, seed=21, flags='random', drop=drop))
        out.append(case(f'flags_row_score_drop{int(drop)}', [65, 9], [5, 1030, 0], [1, 0, 1], seed=22, flags='random',
                        drop=drop, row_score=np.array([0.9, 0.5, 0.1], F32)))
    for dim in ((0, 1, 2), (0, 1, 2, 3, 4), (0, 1, 2, 3, 4, 5), (2, 0, 1, 5), (0, 1, 2, 3, 3), 4):
        out.append(case(f'dim{dim}', [100, 30], [700, 1100], [1, 0], use_dim=dim, seed=15))
    return out


def args_of(c):
    return (c['points'], c['cloud_sizes'], c['occ'], c['counts'], c['frame_rows'], c['use_dim'], c['row_score'], c['flags'],
            c['drop_observed'], c['score_threshold'])
