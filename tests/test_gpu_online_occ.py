"""Completed occupancy from the online steps on the MI355X (TrackletRoIHeadOCC.simple_test_step / simple_test_steps /
simple_test_scene_step with ``occ=True``, OccBBoxHead.get_frame_occ, csrc/occ_frame.hip, tools/online_raw.py --save-occ)
on the small model and the two tracklets of tests/test_gpu_scene_rows.py: 3 slots, 4 frames each under ego motion, the
second tracklet one frame late, one (tracklet, frame) without a point in its box.

A step is not bit-reproducible from run to run, so nothing here compares two runs of the model bit for
bit: every exact comparison takes the latents and the pooled points of the SAME step."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_frame_ref as ref                                                   # noqa: E402
from test_gpu_scene_rows import EMPTY, FRAMES, SLOTS, STARTS, head_frames     # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'ococcnet_mi355x.py')
KEYS = {'boxes', 'scores', 'labels', 'valid', 'fused_roi_feats', 'ori_roi_feats'}
OCC_KEYS = {'occ', 'occ_flags', 'occ_counts'}


@pytest.fixture(scope='module', autouse=True)
def _generators_as_found():
    """later tests of the suite initialise networks from torch's global generators without seeding them"""
    cpu = torch.get_rng_state()
    gpu = torch.cuda.get_rng_state() if torch.cuda.is_available() else None
    yield
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state(gpu)


@pytest.fixture(scope='module')
def model(dev):
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (register)
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    torch.manual_seed(0)
    return DETECTORS.build(ococcnet_model_cfg()).to(dev).eval()


class _HeadTap(object):
    """records (rois, returned dict) of every OccBBoxHead.forward_step / forward_steps call"""

    def __init__(self, head):
        self.head, self.calls = head, []

    def __enter__(self):
        for name in ('forward_step', 'forward_steps'):
            def wrapped(*a, _orig=getattr(self.head, name), **k):
                res = _orig(*a, **k)
                self.calls.append((a[4], res))
                return res
            setattr(self.head, name, wrapped)
        return self

    def __exit__(self, *exc):
        del self.head.forward_step, self.head.forward_steps


def _split(out, key='occ'):
    """the rows of a result per input row: [(xyz-prob [m, 4], flags [m])]"""
    cuts = np.cumsum([0] + list(out['occ_counts']))
    return [(out[key][cuts[r]:cuts[r + 1]], out['occ_flags'][cuts[r]:cuts[r + 1]]) for r in range(len(cuts) - 1)]


@pytest.fixture(scope='module')
def walk(dev, model):
    """the frames of head_frames() through: single steps with occ (fixed-frame rows built by scene_step_rows), scene steps
    with occ, single steps under filter_empty_roi, and two plain twins of the single steps -- once, for the tests below"""
    from objectcentricocccompletion_amd import scene_rows as S
    rh = model.roi_head
    cfg = rh.SCENE_ROWS_DEFAULTS
    st = types.SimpleNamespace(**{k: rh.online_begin(3, dev, cap=FRAMES) for k in ('single', 'scene', 'filt', 'twin1', 'twin2')})
    origin, frames, per_row = {}, [], {}
    for f, (cloud, pose, live) in enumerate(head_frames()):
        points = torch.from_numpy(cloud).to(dev)
        boxes = torch.from_numpy(np.stack([b for _, b, _ in live])).to(dev)
        scores = torch.from_numpy(np.array([s for _, _, s in live], np.float32)).to(dev)
        labels = torch.zeros(len(live), dtype=torch.long, device=dev)
        slot = [SLOTS[t] for t, _, _ in live]
        for t, _, _ in live:
            origin.setdefault(t, np.linalg.inv(pose))
        m64 = np.stack([origin[t] @ pose for t, _, _ in live])
        m32 = torch.from_numpy(m64[:, :3].reshape(-1, 12).astype(np.float32)).to(dev)
        fixed = rh._boxes_through(boxes, torch.from_numpy(m64[:, :3].reshape(-1, 12)).to(dev))
        xyz, feats, row, _ = S.scene_step_rows(points, boxes, scores, transforms=m32, extra_width=cfg['extra_width'],
                                               point_cloud_range=cfg['point_cloud_range'], max_points=cfg['max_points'],
                                               deco_boxes=fixed)
        rec = types.SimpleNamespace(f=f, live=[(t, f - STARTS[t]) for t, _, _ in live], m64=m64, fixed=fixed)
        with _HeadTap(rh.bbox_head) as tap:
            rec.plain_keys = set(rh.simple_test_step(xyz, feats, row, fixed, scores, labels, slot, st.twin1))
            rec.twin1 = tap.calls[-1][1]['fused_roi_feats']
            rec.twin2 = rh.simple_test_step(xyz, feats, row, fixed, scores, labels, slot, st.twin2)['fused_roi_feats']
            rec.single = rh.simple_test_step(xyz, feats, row, fixed, scores, labels, slot, st.single, occ=True)
            rec.single_rois, rec.single_res = tap.calls[-1]
            rec.scene = rh.simple_test_scene_step(points, pose, boxes, scores, labels, slot, st.scene, occ=True)
            rec.scene_rois, rec.scene_res = tap.calls[-1]
            rh.test_cfg['filter_empty_roi'] = True
            try:
                rec.filt = rh.simple_test_step(xyz, feats, row, fixed, scores, labels, slot, st.filt, occ=True)
            finally:
                del rh.test_cfg['filter_empty_roi']
        for r, key in enumerate(rec.live):      # what a later simple_test_steps call needs of (tracklet, frame)
            per_row[key] = types.SimpleNamespace(xyz=xyz[row == r], feats=feats[row == r], box=fixed[r], score=scores[r],
                                                 occ=_split(rec.single)[r], latent=rec.single['fused_roi_feats'][r],
                                                 twins=(rec.twin1[r], rec.twin2[r]))
        frames.append(rec)
    assert st.single.frames == [FRAMES, 0, FRAMES]
    return types.SimpleNamespace(frames=frames, per_row=per_row)


def test_predicted_rows_equal_get_occ_packed(walk, model):
    """at every step the rows with flag bit 0 are get_occ_packed(out['fused_roi_feats'], the step's rois) -- one call for
    all rows of the step, the decode's GEMM shape that of the step -- bit for bit in xyz and counts; the keys are the six
    of today plus three"""
    head = model.roi_head.bbox_head
    cells = 0
    for rec in walk.frames:
        assert rec.plain_keys == KEYS and set(rec.single) == KEYS | OCC_KEYS
        out = rec.single
        assert out['occ'].dtype == torch.float32 and out['occ_flags'].dtype == torch.uint8
        assert out['occ'].shape == (sum(out['occ_counts']), 4) and len(out['occ_counts']) == len(rec.live)
        assert isinstance(out['occ_counts'], list) and all(isinstance(c, int) for c in out['occ_counts'])
        exp, exp_counts = head.get_occ_packed(out['fused_roi_feats'], rec.single_rois)
        pred = (out['occ_flags'] & 1) != 0
        assert torch.equal(out['occ'][pred][:, :3], exp)
        assert [int(((fl & 1) != 0).sum()) for _, fl in _split(out)] == exp_counts
        assert bool(((out['occ_flags'] >= 1) & (out['occ_flags'] <= 3)).all())
        assert bool(((out['occ'][:, 3] > head.occ_ae_head.occ_decoder.pos_thresh) == pred).all())
        cells += int(pred.sum())
    assert cells > 100


def test_observed_rows_are_the_cells_sample_observation_labels(walk, model):
    """the rows with flag bit 1 are exactly the cells OccAutoEncoder.sample_observation labels 1 for the step's pooled
    points, in cell order, through OccDecoder._to_lidar; the row without a point has none"""
    from objectcentricocccompletion_amd.occ.occ_base import OccDecoder
    ae = model.roi_head.bbox_head.occ_ae_head
    seen_rows = 0
    for rec in walk.frames:
        out, rois, res = rec.single, rec.single_rois, rec.single_res
        centers, labels, box = ae.sample_observation(res['local_xyz'], rois, res['roi_inds'], downsample_size=-1,
                                                     balance_sample=False)
        on = labels == 1
        exp = OccDecoder._to_lidar(centers[on], box[on], rois[:, 1:4], rois[:, 4:7], rois[:, 7])
        obs = (out['occ_flags'] & 2) != 0
        assert torch.equal(out['occ'][obs][:, :3], exp)
        per_row = torch.bincount(box[on], minlength=rois.size(0)).tolist()
        assert [int(((fl & 2) != 0).sum()) for _, fl in _split(out)] == per_row
        for r, key in enumerate(rec.live):
            assert (per_row[r] == 0) == (key == EMPTY), (key, per_row[r])
        seen_rows += int(obs.sum())
    assert seen_rows > 200


def test_filter_empty_roi_empties_the_row_without_points(walk):
    hit = False
    for rec in walk.frames:
        for r, key in enumerate(rec.live):
            if key == EMPTY:
                hit = True
                assert rec.filt['occ_counts'][r] == 0 and not bool(rec.filt['valid'][r])
            else:
                assert rec.filt['occ_counts'][r] > 0
        assert rec.filt['occ'].shape == (sum(rec.filt['occ_counts']), 4)
    assert hit


def test_scene_step_occ_ego_goes_back_to_the_fixed_frame_cells(walk, model):
    """simple_test_scene_step(occ=True): ``occ_ego`` in place of ``occ``; flags and counts are those of the fixed-frame
    cells of the same latents and points (OccBBoxHead.get_frame_occ without a matrix), and occ_ego taken back through M_i in
    float64 lies within 3u / (1 - 3u) * (|m0 x| + |m1 y| + |m2 z| + |m3|) per coordinate of them"""
    head = model.roi_head.bbox_head
    worst = 0.0
    for rec in walk.frames:
        out = rec.scene
        assert set(out) == KEYS | {'occ_ego', 'occ_flags', 'occ_counts', 'boxes_ego', 'num_points'}
        fixed, flags, counts = head.get_frame_occ(out['fused_roi_feats'], rec.scene_rois, rec.scene_res['local_xyz'],
                                                  rec.scene_res['roi_inds'])
        assert counts == out['occ_counts'] and torch.equal(flags, out['occ_flags'])
        assert torch.equal(fixed[:, 3], out['occ_ego'][:, 3])
        rows = np.repeat(np.arange(len(counts)), counts)
        m = rec.m64[:, :3].reshape(-1, 12)[rows]
        ego = out['occ_ego'][:, :3].cpu().numpy().astype(np.float64)
        back = (m.reshape(-1, 3, 4)[:, :, :3] * ego[:, None, :]).sum(-1) + m.reshape(-1, 3, 4)[:, :, 3]
        err = np.abs(back - fixed[:, :3].cpu().numpy().astype(np.float64))
        bound = 3 * ref.U / (1 - 3 * ref.U) * ((np.abs(m.reshape(-1, 3, 4)[:, :, :3]) * np.abs(ego)[:, None, :]).sum(-1)
                                             + np.abs(m.reshape(-1, 3, 4)[:, :, 3]))
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (rec.f, float((err / bound).max()))
    print(f'occ_ego back through M in float64: largest error / bound {worst:.3f}')


STEP_ROWS = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 0), (1, 1)]       # (tracklet, frame) of the rows below
SLOT_ROWS = [1, 1, 1, 0, 2, 2]


@pytest.fixture(scope='module')
def chunked(walk, model, dev):
    """simple_test_steps with slot_rows = [1, 1, 1, 0, 2, 2] on fresh states: frames 0-2 of tracklet 0, frame 0 of tracklet
    1, frames 0-1 of tracklet 1 -- once with ``occ``, four times without (existing calls: the yardstick's latents)"""
    rh = model.roi_head
    p = [walk.per_row[k] for k in STEP_ROWS]
    xyz, feats = torch.cat([q.xyz for q in p]), torch.cat([q.feats for q in p])
    row = torch.cat([torch.full((q.xyz.size(0),), i, dtype=torch.long, device=dev) for i, q in enumerate(p)])
    boxes, scores = torch.stack([q.box for q in p]), torch.stack([q.score for q in p])
    labels = torch.zeros(len(p), dtype=torch.long, device=dev)
    plain = [rh.simple_test_steps(xyz, feats, row, boxes, scores, labels, SLOT_ROWS, rh.online_begin(3, dev, cap=FRAMES))
             for _ in range(4)]
    state = rh.online_begin(3, dev, cap=FRAMES)
    out = rh.simple_test_steps(xyz, feats, row, boxes, scores, labels, SLOT_ROWS, state, occ=True)
    assert state.frames == [1, 3, 2]
    return types.SimpleNamespace(p=p, plain=plain, out=out)


def test_steps_select_what_the_single_steps_selected(chunked):
    """against the single steps of the same (tracklet, frame): counts, flags and xyz exact, row by row; without ``occ`` the
    six keys of today"""
    assert all(set(o) == KEYS for o in chunked.plain) and set(chunked.out) == KEYS | OCC_KEYS
    assert len(chunked.out['occ_counts']) == len(SLOT_ROWS)
    for i, ((got, gflags), q) in enumerate(zip(_split(chunked.out), chunked.p)):
        want, wflags = q.occ
        assert got.shape == want.shape and torch.equal(gflags, wflags), STEP_ROWS[i]
        assert torch.equal(got[:, :3], want[:, :3]), STEP_ROWS[i]
    assert sum(chunked.out['occ_counts']) > 100


def test_steps_probabilities_within_what_the_chunk_test_allows_the_latents(chunked):
    """The probabilities of the chunked call against those of the single steps, largest difference over the largest value,
    within the distance tests/test_gpu_online_chunk.py allows the latents: 2 d0 + 1e-7.  There d0 is what EXISTING code gives
    for the same frame at another GEMM row count (an offline prefix against the full pass), over several passes because a
    pass is not bit-reproducible.  Here the same quantity is taken from existing calls only, none with ``occ``: the fused
    latents of four plain simple_test_steps calls (6 rows) and of two plain single-step runs, each against the single
    steps' latents of the same (tracklet, frame).

    THIS CHECK IS MISSED IN SOME RUNS, and is left as the issue states it.  Runs on an MI355X (a step is not
    bit-reproducible, so every run has its own figures):
        probabilities 2.075e-06, chunked latents 1.170e-06, two single-step runs 9.536e-07 apart  (allowed then, from the
                                 two single-step runs alone -- noise at ONE row count, not the chunk test's quantity: 2.007e-06)
        probabilities 2.594e-06, allowed 2.354e-06 (d0 = 1.127e-06 from the plain chunked calls): missed
        probabilities 1.975e-06, chunked latents 9.319e-07, allowed 2.354e-06: held (and held in a run of the whole suite)
    (tests/test_gpu_online_chunk.py printed d0 = 7.166e-07 for the latents of its own tracklet in a run of it: 1.533e-06,
    which the probabilities miss in every run.)
    The selection is exact (the test above) and the latents themselves are inside the allowance; the probability is the
    sigmoid of the bf16 decoder's logit of that latent, and the decoder carries a relative difference of the latent into
    about twice that difference of the probability -- in the chunked call at another row count of its own per-RoI GEMM.
    Nothing in the new code sits between the latent and the probability but the decoder call get_occ_packed makes."""
    p, out = chunked.p, chunked.out
    scale = max(float(q.latent.abs().max()) for q in p)
    d_twin = max(float((tw.double() - q.latent.double()).abs().max()) for q in p for tw in q.twins) / scale
    d_rows = max(float((o['fused_roi_feats'][i].double() - q.latent.double()).abs().max()) for o in chunked.plain
                 for i, q in enumerate(p)) / scale
    d_lat = max(float((out['fused_roi_feats'][i].double() - q.latent.double()).abs().max()) for i, q in enumerate(p)) / scale
    allowed = 2 * max(d_twin, d_rows) + 1e-7
    d_prob = 0.0
    for (got, _), q in zip(_split(out), p):
        want = q.occ[0]
        if got.size(0) and got.shape == want.shape:
            d_prob = max(d_prob, float((got[:, 3].double() - want[:, 3].double()).abs().max()) / float(want[:, 3].abs().max()))
    print(f'steps against single steps: latents {d_lat:.3e}, probabilities {d_prob:.3e}; existing calls: single steps twice '
          f'{d_twin:.3e}, plain chunked calls {d_rows:.3e}, allowed {allowed:.3e}')
    assert d_lat <= allowed, (d_lat, allowed)
    assert d_prob <= allowed, (d_prob, allowed)


def _run(cmd, timeout=600):
    p = subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out, err = p.communicate(timeout=timeout)
    assert p.returncode == 0, out[-2000:] + err[-3000:]
    return out


def test_online_raw_save_occ(dev, model, tmp_path):
    """tools/online_raw.py --save-occ DIR in a child process on make_synthetic_raw's tree (1 segment, 2 objects and a false
    positive, 6 frames): one file per refined object and frame, which occ_export.load_frame_occ reads; the rows in the
    files are the cells the tool counted (its ``occ_counts``, summed and printed); in this process, replay's records carry
    the counts per file, and column 3 is the object's score of the frame"""
    import importlib.util
    from objectcentricocccompletion_amd import occ_export
    tools = os.path.join(ROOT, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import make_synthetic_raw
    root, ckpt = str(tmp_path / 'raw'), str(tmp_path / 'model.pth')
    make_synthetic_raw.main([root, '--segments', '1', '--tracklets', '2', '--frames', '6', '--background', '500'])
    yaml, poses = os.path.join(root, 'synthetic_vehicle.yaml'), os.path.join(root, 'poses.pkl')
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    out_dir = str(tmp_path / 'occ_child')
    stdout = _run(['timeout', '-k', '10', '300', sys.executable, 'tools/online_raw.py', CFG, ckpt, yaml, '--poses', poses,
                   '--slots', '4', '--out', str(tmp_path / 'child.bin'), '--save-occ', out_dir])
    line = [l for l in stdout.splitlines() if 'occupancy cells in' in l][-1]
    printed = int(line.split()[0])
    spec = importlib.util.spec_from_file_location('ococc_tools_online_raw', os.path.join(tools, 'online_raw.py'))
    online_raw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(online_raw)
    here = str(tmp_path / 'occ_here')
    records, state = online_raw.replay(model, yaml, slots=4, poses=poses, save_occ=here)
    assert state.frames == [0, 0, 0, 0] and len(records) >= 12 and all('occ_cells' in r for r in records)
    listing = lambda d: sorted(os.path.relpath(os.path.join(p, n), d) for p, _, names in os.walk(d) for n in names)
    assert listing(out_dir) == listing(here) and len(listing(here)) == len(records)
    rows = 0
    for r in records:
        a = occ_export.read_occ_bin(occ_export.occ_path(here, r['segment'], r['timestamp'], r['type'], r['id']))
        assert a.shape == (r['occ_cells'], 4) and np.isfinite(a).all()
        assert (a[:, 3] == np.float32(r['score'])).all()
        if r['num_points'] > 0:
            assert r['occ_cells'] > 0
    for seg, ts in sorted({(r['segment'], r['timestamp']) for r in records}):
        frame = occ_export.load_frame_occ(out_dir, seg, ts)
        assert frame.dtype == np.float32 and frame.shape[1] == 4 and np.isfinite(frame).all()
        rows += frame.shape[0]
        mine = occ_export.load_frame_occ(here, seg, ts)
        assert mine.shape[0] == sum(r['occ_cells'] for r in records if (r['segment'], r['timestamp']) == (seg, ts))
    assert rows == printed > 0
