"""Waymo-format detection files -- SURVEY 8(f) row 3, the writer / reader side of the tracklet dataset:

  convert_tracklet_to_waymo / lidar2waymo_box   mmdet3d/datasets/waymo_tracklet_dataset.py:430-484
  evaluate (the 'waymo' metric: write the .bin, run compute_detection_metrics_main on it, parse its text)   :315-428
  read_bin / generate_tracklets                 tools/ctrl/utils.py:12-58 (what tools/occ/occ_annotate.py:268-281 reads)

The reference builds ``waymo_open_dataset.protos.metrics_pb2.Objects`` messages.  That package (an un-vendored
dependency of the reference, no version pinned there; the protos below are the published ones of waymo-open-dataset 1.x,
Apache 2.0) is absent from this image, so the messages are encoded and decoded here directly in the protobuf WIRE FORMAT
(varint keys, length-delimited sub-messages, fixed64 doubles, fixed32 floats), field by field:

  metrics.Objects { repeated Object objects = 1; }
  metrics.Object  { Label object = 1; float score = 2; bool overlap_with_nlz = 3; string context_name = 4;
                    int64 frame_timestamp_micros = 5; }
  label.Label     { Box box = 1; Metadata metadata = 2; Type type = 3; string id = 4;
                    DifficultyLevel detection_difficulty_level = 5 (UNKNOWN = 0, LEVEL_1 = 1, LEVEL_2 = 2); ...
                    int32 num_lidar_points_in_box = 7; ...
                    enum Type { TYPE_UNKNOWN = 0; TYPE_VEHICLE = 1; TYPE_PEDESTRIAN = 2; TYPE_SIGN = 3; TYPE_CYCLIST = 4; } }
  label.Label.Box { double center_x = 1; center_y = 2; center_z = 3; width = 4; length = 5; height = 6; heading = 7; }

PARITY UNPINNED for the field numbers: no Waymo proto, file or golden vector exists in /root/reference; the encoder is
pinned to the protobuf LIBRARY for exactly this schema (tests/test_waymo_io_cpu.py builds the schema with
google.protobuf's descriptor pool and compares bytes), the box / heading arithmetic to the reference's call sites.
The metrics binary (mmdet3d/core/evaluation/waymo_utils/compute_detection_metrics_main, a compiled Waymo tool the
reference ships no source for) is not built: `evaluate` writes the .bin and stops there with a clear error unless the
caller names an executable.  The same table computed here, on HIP kernels and with a stated protocol of its own: waymo_metrics.py
(metric 'waymo_native'; tools/waymo_detection_metrics.py has the tool's argv shape and can be that executable)."""
import os
import struct
import subprocess

import numpy as np
import torch

TYPE_UNKNOWN, TYPE_VEHICLE, TYPE_PEDESTRIAN, TYPE_SIGN, TYPE_CYCLIST = 0, 1, 2, 3, 4
K2W_CLS_MAP = {'Car': TYPE_VEHICLE, 'Pedestrian': TYPE_PEDESTRIAN, 'Sign': TYPE_SIGN, 'Cyclist': TYPE_CYCLIST}  # :113-118


# ------------------------------------------------------------------------------------------------ wire format
def _varint(v):
    v &= (1 << 64) - 1          # negative int64 -> ten-byte two's complement, as protobuf writes it
    out = bytearray()
    while True:
        b = v & 0x7f
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _key(field, wire):
    return _varint((field << 3) | wire)


def _f_double(field, v):
    return _key(field, 1) + struct.pack('<d', float(v))


def _f_float(field, v):
    return _key(field, 5) + struct.pack('<f', float(v))


def _f_varint(field, v):
    return _key(field, 0) + _varint(int(v))


def _f_bytes(field, b):
    return _key(field, 2) + _varint(len(b)) + b


def _read_varint(buf, pos):
    shift = v = 0
    while True:
        b = buf[pos]
        pos += 1
        v |= (b & 0x7f) << shift
        if not b & 0x80:
            return v, pos
        shift += 7


def _fields(buf):
    """(field number, wire type, value) of every field of one message; value: int (varint), bytes (fixed / delimited)"""
    pos, n = 0, len(buf)
    while pos < n:
        key, pos = _read_varint(buf, pos)
        field, wire = key >> 3, key & 7
        if wire == 0:
            v, pos = _read_varint(buf, pos)
        elif wire == 1:
            v, pos = buf[pos:pos + 8], pos + 8
        elif wire == 5:
            v, pos = buf[pos:pos + 4], pos + 4
        elif wire == 2:
            ln, pos = _read_varint(buf, pos)
            v, pos = buf[pos:pos + ln], pos + ln
        else:
            raise ValueError(f'unsupported wire type {wire}')
        yield field, wire, v


# ------------------------------------------------------------------------------------------------ writer
def lidar2waymo_box(in_box, score, waymo_type, context_name, timestamp, object_id=None, overlap_with_nlz=None,
                    detection_difficulty_level=None, num_lidar_points_in_box=None):
    """One box [7] (x, y, z_bottom, w, l, h, yaw; LiDAR box convention of the reference) -> the serialised
    metrics.Object, following waymo_tracklet_dataset.py:455-484 number for number (including its 3.1415926 / 3.141593 /
    3.141592 constants).  The three optional fields (Object.overlap_with_nlz = 3, Label.detection_difficulty_level = 5,
    Label.num_lidar_points_in_box = 7: what a ground-truth file carries for waymo_metrics) are written in field-number
    order whenever given (proto2 presence: an explicit 0 / False is on the wire, as the protobuf library writes a set
    optional field); left out, the bytes are the reference's."""
    b = [float(v) for v in in_box]
    height = b[5]
    heading = -b[6] - 0.5 * 3.1415926
    while heading < -3.141593:
        heading += 2 * 3.141592
    while heading > 3.141593:
        heading -= 2 * 3.141592
    box = (_f_double(1, b[0]) + _f_double(2, b[1]) + _f_double(3, b[2] + height / 2) + _f_double(4, b[3]) +
           _f_double(5, b[4]) + _f_double(6, height) + _f_double(7, heading))
    label = _f_bytes(1, box) + _f_varint(3, waymo_type)
    if object_id is not None:
        label += _f_bytes(4, str(object_id).encode())
    if detection_difficulty_level is not None:
        label += _f_varint(5, int(detection_difficulty_level))
    if num_lidar_points_in_box is not None:
        label += _f_varint(7, int(num_lidar_points_in_box))
    nlz = b'' if overlap_with_nlz is None else _f_varint(3, bool(overlap_with_nlz))
    return (_f_bytes(1, label) + _f_float(2, score) + nlz + _f_bytes(4, str(context_name).encode()) +
            _f_varint(5, int(timestamp)))


def convert_tracklet_to_waymo(tracklets, pkl_path, classes=('Car', 'Pedestrian', 'Cyclist'), overlap_with_nlz=None,
                              detection_difficulty_level=None, num_lidar_points_in_box=None):
    """tracklets (tracklet.Tracklet with ``type`` = index into ``classes``, string ``id``, ``segment_name``) -> the
    metrics.Objects file ``pkl_path`` (+ '.bin'), waymo_tracklet_dataset.py:430-453.  Returns the path written.
    The three optional arguments (see lidar2waymo_box) are one sequence per tracklet with one value per box, or None."""
    per_box = lambda seq, k, i: None if seq is None else seq[k][i]
    chunks = []
    for k, trk in enumerate(tracklets):
        assert isinstance(trk.id, str)
        wtype = K2W_CLS_MAP[classes[trk.type]]
        boxes = trk.boxes.detach().cpu().numpy()
        scores = trk.scores.detach().cpu().numpy()
        for i in range(len(trk)):
            chunks.append(_f_bytes(1, lidar2waymo_box(
                boxes[i], scores[i], wtype, trk.segment_name, trk.ts_list[i], trk.id, per_box(overlap_with_nlz, k, i),
                per_box(detection_difficulty_level, k, i), per_box(num_lidar_points_in_box, k, i))))
    if not pkl_path.endswith('.bin'):
        pkl_path += '.bin'
    with open(pkl_path, 'wb') as f:
        f.write(b''.join(chunks))
    return pkl_path


def write_objects(records, path):
    """The inverse of read_bin: its records (dicts) -> the metrics.Objects file ``path``, every field as it was read --
    the box stays in the Waymo convention (centre, length / width / height, heading: no conversion), the score is a
    32-bit float on the wire, fields in field-number order as the protobuf library writes them.  read_bin does not
    record presence, so the three optional ground-truth fields and the id are written where they differ from the
    reader's defaults (False / 0 / 0 / ''): a file read, written and read again gives equal records, and a file of
    convert_tracklet_to_waymo without explicit zeros in those fields gives equal bytes.  Returns ``path``."""
    chunks = []
    for o in records:
        box = b''.join(_f_double(i + 1, o[k]) for i, k in enumerate(
            ('center_x', 'center_y', 'center_z', 'width', 'length', 'height', 'heading')))
        label = _f_bytes(1, box) + _f_varint(3, o['type'])
        if o['id'] != '':
            label += _f_bytes(4, str(o['id']).encode())
        if o['detection_difficulty_level']:
            label += _f_varint(5, int(o['detection_difficulty_level']))
        if o['num_lidar_points_in_box']:
            label += _f_varint(7, int(o['num_lidar_points_in_box']))
        nlz = _f_varint(3, True) if o['overlap_with_nlz'] else b''
        chunks.append(_f_bytes(1, _f_bytes(1, label) + _f_float(2, o['score']) + nlz +
                               _f_bytes(4, str(o['context_name']).encode()) + _f_varint(5, int(o['frame_timestamp_micros']))))
    with open(path, 'wb') as f:
        f.write(b''.join(chunks))
    return path


# ------------------------------------------------------------------------------------------------ reader
def read_bin(file_path):
    """tools/ctrl/utils.py:12-16 -> list of dicts (box fields, type, id, score, context_name, frame_timestamp_micros,
    and overlap_with_nlz / detection_difficulty_level / num_lidar_points_in_box, False / 0 / 0 where absent)"""
    with open(file_path, 'rb') as f:
        buf = f.read()
    out = []
    for field, wire, obj in _fields(buf):
        if field != 1 or wire != 2:
            continue
        rec = dict(score=0.0, context_name='', frame_timestamp_micros=0, type=0, id='', center_x=0.0, center_y=0.0,
                   center_z=0.0, width=0.0, length=0.0, height=0.0, heading=0.0, overlap_with_nlz=False,
                   detection_difficulty_level=0, num_lidar_points_in_box=0)
        for f2, w2, v2 in _fields(obj):
            if f2 == 1 and w2 == 2:
                for f3, w3, v3 in _fields(v2):
                    if f3 == 1 and w3 == 2:
                        names = {1: 'center_x', 2: 'center_y', 3: 'center_z', 4: 'width', 5: 'length', 6: 'height', 7: 'heading'}
                        for f4, w4, v4 in _fields(v3):
                            if w4 == 1 and f4 in names:
                                rec[names[f4]] = struct.unpack('<d', v4)[0]
                    elif f3 == 3 and w3 == 0:
                        rec['type'] = v3
                    elif f3 == 4 and w3 == 2:
                        rec['id'] = v3.decode()
                    elif f3 == 5 and w3 == 0:
                        rec['detection_difficulty_level'] = v3
                    elif f3 == 7 and w3 == 0:
                        rec['num_lidar_points_in_box'] = (v3 & 0xffffffff) - (1 << 32) if v3 & 0x80000000 else v3 & 0xffffffff
            elif f2 == 2 and w2 == 5:
                rec['score'] = struct.unpack('<f', v2)[0]
            elif f2 == 3 and w2 == 0:
                rec['overlap_with_nlz'] = bool(v2)
            elif f2 == 4 and w2 == 2:
                rec['context_name'] = v2.decode()
            elif f2 == 5 and w2 == 0:
                rec['frame_timestamp_micros'] = v2 - (1 << 64) if v2 >> 63 else v2
        out.append(rec)
    return out


def generate_tracklets(objects, types=None):
    """tools/ctrl/utils.py:18-58: the objects of a metrics file -> one tracklet per (segment, object id), boxes back in
    the LiDAR convention (z at the bottom face, w / l swapped, heading -> yaw wrapped into [-pi, pi]), frames sorted by
    timestamp (LiDARTracklet.freeze)."""
    from .tracklet import Tracklet
    if types is None:
        types = (1, 2, 4)
    acc = {}
    for o in objects:
        if o['type'] not in types:
            continue
        heading = -o['heading'] - 0.5 * np.pi
        while heading < -np.pi:
            heading += 2 * np.pi
        while heading > np.pi:
            heading -= 2 * np.pi
        box = np.array([o['center_x'], o['center_y'], o['center_z'] - o['height'] / 2, o['width'], o['length'], o['height'],
                        heading], dtype=np.float32)
        key = o['context_name'] + '-' + o['id']
        acc.setdefault(key, dict(seg=o['context_name'], id=o['id'], type=o['type'], rows=[]))['rows'].append(
            (o['frame_timestamp_micros'], box, o['score']))
    out = []
    for rec in acc.values():
        rows = sorted(rec['rows'], key=lambda r: r[0])
        t = Tracklet(torch.from_numpy(np.stack([r[1] for r in rows], 0)), [r[0] for r in rows],
                     torch.tensor([r[2] for r in rows], dtype=torch.float32), rec['type'], rec['seg'], rec['id'])
        t.in_world, t.type_format = False, 'waymo'
        out.append(t)
    return out


# ------------------------------------------------------------------------------------------------ the 'waymo' metric
AP_KEYS = [f'{c}/{lvl} {m}' for c in ('Vehicle', 'Pedestrian', 'Sign', 'Cyclist') for lvl in ('L1', 'L2') for m in ('mAP', 'mAPH')]


def parse_detection_metrics(text):
    """The text compute_detection_metrics_main prints -> the reference's ap_dict (waymo_tracklet_dataset.py:375-419):
    the i-th 'mAP ' / 'mAPH ' occurrence, up to the closing bracket, in the tool's object-type / level order; the
    'Overall' entries average Vehicle, Pedestrian and Cyclist."""
    ap = {k: 0.0 for k in AP_KEYS}
    ap.update({f'Overall/{lvl} {m}': 0.0 for lvl in ('L1', 'L2') for m in ('mAP', 'mAPH')})
    m_ap, m_aph = text.split('mAP '), text.split('mAPH ')
    for idx, key in enumerate(AP_KEYS):
        split_idx = idx // 2 + 1
        ap[key] = float((m_ap if idx % 2 == 0 else m_aph)[split_idx].split(']')[0])
    for lvl in ('L1', 'L2'):
        for m in ('mAP', 'mAPH'):
            ap[f'Overall/{lvl} {m}'] = (ap[f'Vehicle/{lvl} {m}'] + ap[f'Pedestrian/{lvl} {m}'] + ap[f'Cyclist/{lvl} {m}']) / 3
    return ap


def evaluate(results, pklfile_prefix, gt_bin, classes=('Car', 'Pedestrian', 'Cyclist'), metrics_main=None):
    """WaymoTrackletDataset.evaluate (:315-428): results (refined tracklets) -> ``pklfile_prefix``.bin, then the Waymo
    tool on it against ``gt_bin``.  ``metrics_main``: path of compute_detection_metrics_main; the tool is a compiled
    binary of waymo-open-dataset that is not part of this repository -- without it the .bin is written and a
    RuntimeError names what is missing (the stated stop of SURVEY 8(f) row 3)."""
    path = convert_tracklet_to_waymo(results, pklfile_prefix, classes)
    if metrics_main is None or not os.path.isfile(metrics_main):
        raise RuntimeError(f'wrote {path}; the Waymo metrics tool (compute_detection_metrics_main) is not available '
                           f'here -- run it on {path} {gt_bin} and pass its output to waymo_io.parse_detection_metrics')
    text = subprocess.check_output([metrics_main, path, gt_bin]).decode('utf-8')
    with open(f'{pklfile_prefix}.txt', 'w') as fw:
        fw.write(text)
    return parse_detection_metrics(text)
