"""Empty-box removal on the MI355X: the non-empty mode of csrc/tracklet_crop.hip (ctrl_prep.nonempty_frames_packed,
ctrl_prep.remove_empty) and, end to end, tools/ctrl/extend_tracks.py -> tools/ctrl/remove_empty.py ->
tools/ctrl/generate_track_input.py on the synthetic raw tree.

Yardsticks: the parent's count kernel (flags == counts > 0, bit for bit: the same membership arithmetic), and a float64
membership test written here on scenes where no point lies within 1e-3 m of a box face (checked on the CPU first)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def in_box_f64(xyz, box):
    """check_pt_in_box3d (points_in_boxes_cuda.cu:24-49) in float64; box: x, y, z_bottom, w, l, h, yaw"""
    xyz, box = np.asarray(xyz, np.float64), np.asarray(box, np.float64)
    x, y, zb, w, l, h, yaw = box[:7]
    rot = yaw + np.pi / 2
    dx, dy = xyz[:, 0] - x, xyz[:, 1] - y
    lx = dx * np.cos(rot) - dy * np.sin(rot)
    ly = dx * np.sin(rot) + dy * np.cos(rot)
    return (np.abs(xyz[:, 2] - (zb + h / 2)) <= h / 2) & (lx > -l / 2) & (lx < l / 2) & (ly > -w / 2) & (ly < w / 2)


def grown(box, e):
    b = np.asarray(box, np.float64).copy()
    b[3:6] += 2 * e
    b[2] -= e
    return b


def in_shell(xyz, box, e=1e-3):
    return in_box_f64(xyz, grown(box, e)) & ~in_box_f64(xyz, grown(box, -e))


def undecided(xyz, box, e=1e-3):
    """the box's flag hangs on points within e of a face: a point in the box grown by e, none in the box shrunk by e
    (a box with a point in the shrunk box is non-empty, one without a point in the grown box empty, whatever float32
    rounding does to the faces)"""
    return bool(in_box_f64(xyz, grown(box, e)).any()) and not bool(in_box_f64(xyz, grown(box, -e)).any())


def lifted_f64(rec, lift):
    """a record of read_bin -> the lifted LiDAR box in float64: bottom centre, (width, length, height), yaw"""
    h = rec['height']
    return np.array([rec['center_x'], rec['center_y'], rec['center_z'] - h / 2 + lift * h, rec['width'], rec['length'], h,
                     -rec['heading'] - np.pi / 2])


# ---------------------------------------------------------------------------------------------- flags == counts > 0
def flag_scene(seed=3):
    """7 frames: 100 boxes on 60 000 points, no boxes, no points, 70 boxes on 5 000 points, small ones; half of the
    boxes of a frame sit on points, the others above or far from every point"""
    rng = np.random.default_rng(seed)
    sizes = [60_000, 20_000, 0, 5_000, 4_097, 64, 9_000]
    num_boxes = [100, 0, 7, 70, 65, 3, 1]
    points, boxes = [], []
    for n, nb in zip(sizes, num_boxes):
        xyz = rng.uniform([-75, -75, -2], [75, 75, 4], (n, 3))
        bx = np.stack([rng.uniform(-70, 70, nb), rng.uniform(-70, 70, nb), rng.uniform(-1.5, 1.0, nb), rng.uniform(0.5, 2.4, nb),
                       rng.uniform(0.6, 5.5, nb), rng.uniform(0.8, 2.0, nb), rng.uniform(-np.pi, np.pi, nb)], 1)
        bx[nb // 2:, 2] += rng.choice([8.0, 30.0], nb - nb // 2)
        if n and nb:
            own = rng.integers(0, nb // 2 + 1, n // 20)               # a few points right at some box centres
            xyz[:len(own)] = bx[own, :3] + [0, 0, 0.4] + rng.normal(0, 0.3, (len(own), 3))
        points.append(np.concatenate([xyz, rng.random((n, 3))], 1).astype(np.float32))
        boxes.append(bx.astype(np.float32))
    return points, boxes


def packed(points, boxes, dev):
    po = np.concatenate([[0], np.cumsum([len(p) for p in points])]).tolist()
    bo = np.concatenate([[0], np.cumsum([len(b) for b in boxes])]).tolist()
    return torch.from_numpy(np.concatenate(points, 0)).to(dev), po, torch.from_numpy(np.concatenate(boxes, 0)).to(dev), bo


def test_flags_equal_count_kernel(dev):
    from objectcentricocccompletion_amd import ctrl_prep as cp
    points, boxes = flag_scene()
    assert max(len(b) for b in boxes) > 64 and max(len(p) for p in points) > 4096
    args = packed(points, boxes, dev)
    counts, _ = cp.crop_frames_packed(*args)
    flags = cp.nonempty_frames_packed(*args)
    again = cp.nonempty_frames_packed(*args)
    assert flags.dtype == torch.int32 and flags.shape == (sum(len(b) for b in boxes),)
    got = flags.cpu().numpy()
    print(f'non-empty flags: {int(got.sum())} of {len(got)} boxes hold a point; the count kernel says {int((counts > 0).sum())}')
    assert np.array_equal(got, (counts.numpy() > 0).astype(np.int32))
    assert got.tobytes() == again.cpu().numpy().tobytes()
    assert 20 < got.sum() < len(got) - 20
    assert got[100:107].sum() == 0          # the frame without points


# ---------------------------------------------------------------------------------------------- constructed scene
def constructed_scene(seed=9, lift=0.2):
    """Records in the Waymo convention on a grid (no two boxes near each other), points at chosen box-local places at
    least 5 cm from every face of the LIFTED box -> (records per frame, clouds per frame, expected flags per frame,
    kinds).  Kinds: 0 points inside the lifted box; 1 points only in the bottom `lift * h` slab (empty BECAUSE of the
    lift); 2 points only between the old and the lifted top (non-empty BECAUSE of the lift); 3 no point nearby;
    4 points just outside a side face."""
    rng = np.random.default_rng(seed)
    frames, clouds, expect, kinds = [], [], [], []
    for f in range(3):
        recs, pts, exp, kind = [], [], [], []
        nb = [90, 12, 30][f]
        for b in range(nb):
            gx, gy = (b % 10) * 14.0 - 63.0, (b // 10) * 14.0 - 63.0
            w, l, h = rng.uniform(1.6, 2.4), rng.uniform(3.8, 5.5), rng.uniform(1.4, 2.0)
            rec = dict(center_x=gx + rng.uniform(-1, 1), center_y=gy + rng.uniform(-1, 1), center_z=rng.uniform(0.5, 1.5), width=w,
                       length=l, height=h, heading=rng.uniform(-np.pi, np.pi))
            k = b % 5
            n = int(rng.integers(1, 6))
            u = rng.uniform(-0.45, 0.45, (n, 2))                   # fractions of (l, w) along the lifted box's local axes
            if k == 0:
                z = rng.uniform(-0.5 * h + lift * h + 0.05, 0.5 * h + lift * h - 0.05, n)
            elif k == 1:
                z = rng.uniform(-0.5 * h + 0.05, -0.5 * h + lift * h - 0.05, n)
            elif k == 2:
                z = rng.uniform(0.5 * h + 0.05, 0.5 * h + lift * h - 0.05, n)
            elif k == 3:
                z = np.full(n, 25.0)
            else:
                z = rng.uniform(-0.3 * h + lift * h, 0.3 * h + lift * h, n)
                u[:, 0] = 0.5 + 0.05 / l + rng.uniform(0, 0.05, n)  # beyond the front face
            rot = -rec['heading'] - np.pi / 2 + np.pi / 2          # the membership test turns by yaw + pi / 2
            lx, ly = u[:, 0] * l, u[:, 1] * w                      # lx = dx cos - dy sin, ly = dx sin + dy cos
            dx, dy = lx * np.cos(rot) + ly * np.sin(rot), -lx * np.sin(rot) + ly * np.cos(rot)
            pts.append(np.stack([rec['center_x'] + dx, rec['center_y'] + dy, rec['center_z'] + z], 1))
            recs.append(rec)
            exp.append(k in (0, 2))
            kind.append(k)
        frames.append(recs)
        clouds.append(np.concatenate(pts, 0).astype(np.float32)[rng.permutation(sum(len(p) for p in pts))])
        expect.append(np.asarray(exp))
        kinds.append(np.asarray(kind))
    return frames, clouds, expect, kinds


def test_flags_exact_on_constructed_scene(dev):
    from objectcentricocccompletion_amd import ctrl_prep as cp
    lift = cp.BOTTOM_LIFT['vehicle']
    frames, clouds, expect, kinds = constructed_scene(lift=lift)
    # on the CPU, before the GPU is touched: no point within 1e-3 of any face, and the float64 test gives the constructed flags
    for recs, cloud, exp in zip(frames, clouds, expect):
        for rec, e in zip(recs, exp):
            box = lifted_f64(rec, lift)
            assert not in_shell(cloud, box).any()
            assert bool(in_box_f64(cloud, box).any()) == bool(e)
    assert all(set(k.tolist()) == {0, 1, 2, 3, 4} for k in kinds)
    boxes = [cp.lifted_lidar_boxes(recs, lift).numpy() for recs in frames]
    points = [np.concatenate([c, np.zeros((len(c), 3), np.float32)], 1) for c in clouds]
    flags = cp.nonempty_frames_packed(*packed(points, boxes, dev)).cpu().numpy().astype(bool)
    exp = np.concatenate(expect)
    kind = np.concatenate(kinds)
    print('constructed scene: boxes kept per kind (inside, bottom slab only, lifted top only, nothing, beside): '
          + ', '.join(f'{int(flags[kind == k].sum())}/{int((kind == k).sum())}' for k in range(5)))
    assert len(flags) == len(exp) == 132
    assert np.array_equal(flags, exp)


# ---------------------------------------------------------------------------------------------- end to end
def _run(cmd, timeout):
    """a fresh child process under its own time limit; its exit status is checked before the next one starts"""
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def test_extend_then_remove_empty_end_to_end(tmp_path, dev):
    import yaml
    from objectcentricocccompletion_amd import ctrl_prep as cp
    from objectcentricocccompletion_amd import waymo_io
    raw = str(tmp_path / 'raw')
    _run([sys.executable, 'tools/make_synthetic_raw.py', raw], 300)
    pred = os.path.join(raw, 'waymo_format', 'pred.bin')
    _run([sys.executable, 'tools/ctrl/extend_tracks.py', os.path.join(raw, 'synthetic_extend.yaml')], 600)
    extended = os.path.join(raw, 'waymo_format', 'pred_synthetic_extend.bin')
    before, after = waymo_io.read_bin(pred), waymo_io.read_bin(extended)

    # every original (segment, id, timestamp) plus the planned extras
    ext_cfg = yaml.safe_load(open(os.path.join(raw, 'synthetic_extend.yaml')))
    ts2idx, seg_ts = cp.load_frame_index(os.path.join(raw, 'kitti_format'))
    key = lambda o: (o['context_name'], o['id'], o['frame_timestamp_micros'])
    planned = set(key(o) for o in before)
    by_track = {}
    for o in before:
        by_track.setdefault((o['context_name'], o['id']), []).append(o['frame_timestamp_micros'])
    extras = 0
    for (seg, tid), stamps in by_track.items():
        stamps = sorted(stamps)
        if len(stamps) < ext_cfg['min_length_to_extend'] or len(stamps) < 2 or stamps[1] - stamps[0] > 500_000:
            continue
        first = seg_ts[seg].index(stamps[0])
        for ts in seg_ts[seg][first - min(ext_cfg['extend_length'], first):first]:
            planned.add((seg, tid, ts))
            extras += 1
    print(f'extension: {len(before)} objects -> {len(after)}, {extras} planned extras')
    assert extras > 0 and len(after) == len(before) + extras
    assert sorted(key(o) for o in after) == sorted(planned)
    old = {key(o): o for o in before}
    for o in after:                    # observed boxes come back from the shared frame where they were: float32 round trip
        if key(o) in old:
            p = old[key(o)]
            assert o['score'] == p['score'] and o['type'] == p['type']
            assert abs(o['center_x'] - p['center_x']) < 1e-4 and abs(o['center_y'] - p['center_y']) < 1e-4

    _run([sys.executable, 'tools/ctrl/remove_empty.py', '--bin-path', extended, '--split', 'training', '--type', 'vehicle',
          '--mm-data-root', os.path.join(raw, 'kitti_format'), '--gt-bin', os.path.join(raw, 'waymo_format', 'gt.bin')], 600)
    filtered = os.path.join(raw, 'waymo_format', 'pred_synthetic_extend_wo_empty_right.bin')
    assert os.path.isfile(filtered.replace('.bin', '.txt'))
    kept = waymo_io.read_bin(filtered)
    # a subset with unchanged records, in the file's frame order
    pool = {}
    for o in after:
        pool[key(o)] = o
    assert all(pool[key(o)] == o for o in kept) and len(set(key(o) for o in kept)) == len(kept)
    kept_keys = set(key(o) for o in kept)
    order = {ts: i for i, ts in enumerate(dict.fromkeys(o['frame_timestamp_micros'] for o in after))}
    assert [order[o['frame_timestamp_micros']] for o in kept] == sorted(order[o['frame_timestamp_micros']] for o in kept)
    # every kept box has a point, every dropped one has none, by the float64 test; boxes whose flag hangs on points in the 1e-3 shell excepted
    lift, unsure, wrong = cp.BOTTOM_LIFT['vehicle'], 0, []
    clouds = {}
    for o in after:
        ts = o['frame_timestamp_micros']
        if ts not in clouds:
            clouds[ts] = np.fromfile(os.path.join(raw, 'kitti_format', 'training', 'velodyne', ts2idx[ts] + '.bin'), np.float32).reshape(-1, 6)[:, :3]
        box = lifted_f64(o, lift)
        if undecided(clouds[ts], box):
            unsure += 1
        elif bool(in_box_f64(clouds[ts], box).any()) != (key(o) in kept_keys):
            wrong.append(key(o))
    print(f'remove_empty: {len(kept)} of {len(after)} boxes kept; {unsure} boxes undecided within the 1e-3 m shell '
          f'({100 * unsure / len(after):.2f} %)')
    assert unsure <= 0.02 * len(after)
    assert not wrong
    assert 0 < len(kept) < len(after)
    assert not any(o['id'].endswith('_fp') for o in kept)       # the false positives float above every point

    # the next step of the recipe reads the filtered file
    cfg = yaml.safe_load(open(os.path.join(raw, 'synthetic_vehicle.yaml')))
    cfg['bin_path'] = filtered
    with open(os.path.join(raw, 'filtered_vehicle.yaml'), 'w') as f:
        yaml.safe_dump(cfg, f, sort_keys=False)
    _run([sys.executable, 'tools/ctrl/generate_track_input.py', os.path.join(raw, 'filtered_vehicle.yaml')], 600)
    infos = pickle.load(open(os.path.join(raw, 'tracklet_data', 'filtered_vehicle_training.pkl'), 'rb'))
    assert sum(len(e[5]) for e in infos) == len(kept) and all(min(e[7]) > 0 for e in infos)
