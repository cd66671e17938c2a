"""Completed-occupancy files: what TrackletRoIHeadOCC.save_occ_from_tracklet writes and what a detector reads back
(mmdet3d/models/roi_heads/tracklet_roi_head_occ.py:719-744).

Layout: ``<root>/<segment>/<timestamp>/<type>_<id>.bin``, one file per object and frame: float32 [n, 4], row-major,
the occupied cell centres in the LiDAR frame of that timestamp and a score column (the frame's box score in every row).
A frame without occupied cells is an empty file."""
import os

import numpy as np


def occ_path(root, segment, ts, type, id):
    """The reference's f"{occ_save_root}/{segment_name}/{ts}/{type}_{id}.bin"."""
    return os.path.join(f'{root}/{segment}/{ts}', f'{type}_{id}.bin')


def write_tracklet_occ(root, segment, ts_list, type, id, packed, counts, skip=None):
    """Cut ``packed`` ([sum counts, 4] float32 in host memory, frame after frame) into one file per frame of one
    tracklet; frames whose index is in ``skip`` are not written.  Returns the paths written."""
    packed = np.ascontiguousarray(packed, dtype=np.float32)
    assert packed.ndim == 2 and packed.shape[1] == 4, packed.shape
    assert len(counts) == len(ts_list), f'{len(counts)} != {len(ts_list)}'
    assert int(sum(counts)) == packed.shape[0], f'{sum(counts)} != {packed.shape[0]}'
    skip = set(skip or ())
    paths, row = [], 0
    for i, (ts, n) in enumerate(zip(ts_list, counts)):
        rows, row = packed[row:row + n], row + n
        if i in skip:
            continue
        path = occ_path(root, segment, ts, type, id)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        rows.tofile(path)
        paths.append(path)
    return paths


def read_occ_bin(path):
    """One file -> float32 [n, 4]."""
    return np.fromfile(path, dtype=np.float32).reshape(-1, 4)


def load_frame_occ(root, segment, ts, types=None):
    """All objects of one frame, concatenated in sorted file-name order: float32 [m, 4], the array a detector appends to
    the frame's point cloud.  ``types``: keep only the objects of these types (the ``<type>`` of the file names)."""
    folder = f'{root}/{segment}/{ts}'
    names = sorted(n for n in os.listdir(folder) if n.endswith('.bin')) if os.path.isdir(folder) else []
    if types is not None:
        types = {str(t) for t in types}
        names = [n for n in names if n[:-4].split('_', 1)[0] in types]
    parts = [read_occ_bin(os.path.join(folder, n)) for n in names]
    return np.concatenate(parts, 0) if parts else np.zeros((0, 4), np.float32)


def occ_pred_filename(root, segment, ts, per_object_occ):
    """What WaymoDatasetWithPredOCC.get_data_info puts into results['occ_pred_filename']
    (mmdet3d/datasets/waymo_dataset.py:1572-1575): the frame's directory of per-object files -- the layout above -- with
    ``per_object_occ``, else one file ``<root>/<segment>/<timestamp>.bin`` per frame."""
    return os.path.join(root, segment, f'{ts}' if per_object_occ else f'{ts}.bin')
