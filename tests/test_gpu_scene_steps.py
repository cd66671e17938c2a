"""Several sensor frames per online call on the MI355X: TrackletRoIHeadOCC.simple_test_scene_steps and
tools/online_raw.py --chunk.

The head: the scene of test_gpu_scene_rows.test_head_scene_step_matches_the_existing_operators (two tracklets of 4 frames
under ego motion, the second a frame late, one (tracklet, frame) without a point) fed as TWO calls with slot-major rows,
the second tracklet starting inside the first call.  The reference builds the same rows per frame with the existing
scene_step_rows and _boxes_through and gives them to the existing simple_test_steps on a second state, same row grouping.
The tool: make_synthetic_raw's tree replayed with chunk = 3 and chunk = 1."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_rows_ref as R        # noqa: E402
import scene_steps_ref as RS      # noqa: E402
from test_gpu_scene_rows import EMPTY, FRAMES, SLOTS, STARTS, head_frames     # noqa: E402
from objectcentricocccompletion_amd import _lib as L        # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ((0, 1, 2), (3, 4))          # the sensor frames of the two calls
KEYS = {'boxes', 'scores', 'labels', 'valid', 'fused_roi_feats', 'ori_roi_feats', 'boxes_ego', 'num_points'}
OCC_KEYS = {'occ_ego', 'occ_flags', 'occ_counts'}
CLOSE = ('boxes', 'scores', 'fused_roi_feats')
# The seed of the model's random weights.  The occupancy test asks that no decoder logit of the reference call lie within
# 1e-3 of the decision threshold (logit 0).  Measured on an MI355X over the seeds 0..39, 14 080 logits each: every seed whose
# logits straddle the threshold has one within 4e-4 of it (seed 0: 5.6e-5); the seeds that pass are those whose decoder
# bias puts all logits on one side -- 1, 3, 6, 9, 24, 32 (none predicted: the 634 observed cells only) and 7, 19, 20, 34,
# 35 (all predicted).  Seed 7: logits in [0.263, 0.908], every one of the 14 080 cells of the 8 rows a row of occ_ego,
# flags 1 and 3.
MODEL_SEED = 7


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


@pytest.fixture(scope='module')
def model(dev):
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (register)
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    torch.manual_seed(MODEL_SEED)
    return DETECTORS.build(ococcnet_model_cfg()).to(dev).eval()


def call_inputs(dev, frames, fs, origin):
    """the arguments of one simple_test_scene_steps call over the sensor frames ``fs``: rows slot-major (tracklet 0's frames,
    then tracklet 1's), and per row the float64 matrix into its slot's fixed frame"""
    rows = [(t, j, f, box, score) for t in range(len(STARTS)) for j, f in enumerate(fs)
            for tt, box, score in frames[f][2] if tt == t]
    for t, _, f, _, _ in rows:
        origin.setdefault(t, np.linalg.inv(frames[f][1]))
    clouds = [frames[f][0] for f in fs]
    return dict(points=torch.from_numpy(np.concatenate(clouds)).to(dev), cloud_sizes=[len(c) for c in clouds],
                poses=np.stack([frames[f][1] for f in fs]),
                boxes=torch.from_numpy(np.stack([b for *_, b, _ in rows])).to(dev),
                scores=torch.from_numpy(np.array([s for *_, s in rows], np.float32)).to(dev),
                labels=torch.zeros(len(rows), dtype=torch.long, device=dev),
                frame_rows=[j for _, j, _, _, _ in rows], slot_rows=[SLOTS[t] for t, *_ in rows]), \
        np.stack([origin[t] @ frames[f][1] for t, _, f, _, _ in rows]), [(t, f - STARTS[t]) for t, _, f, _, _ in rows]


def through(occ, m12, counts):
    """cells [N, 4] through the per-row f32 matrices m12 [n, 12], every operation rounded once to f32, in the order of the
    fill kernel of csrc/occ_export.hip: ((m0 x + m1 y) + m2 z) + m3"""
    m = m12[torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts)).to(occ.device)]
    x, y, z = occ[:, 0], occ[:, 1], occ[:, 2]
    cols = [torch.add(torch.add(torch.add(torch.mul(m[:, 4 * c], x), torch.mul(m[:, 4 * c + 1], y)), torch.mul(m[:, 4 * c + 2], z)),
                      m[:, 4 * c + 3]) for c in range(3)]
    return torch.stack(cols, 1)


class _StepsTap(object):
    """records (rois, returned dict) of every OccBBoxHead.forward_steps call"""

    def __init__(self, head):
        self.head, self.calls = head, []

    def __enter__(self):
        orig = self.head.forward_steps

        def wrapped(*a, **k):
            res = orig(*a, **k)
            self.calls.append((a[4], res))
            return res
        self.head.forward_steps = wrapped
        return self

    def __exit__(self, *exc):
        del self.head.forward_steps


def assert_occ_of_own_latents(head, out, rois, res, inv32):
    """the three occ keys of a simple_test_scene_steps result against OccBBoxHead.get_frame_occ (no matrix) on the SAME
    call's fused latents and pooled points, which is deterministic: counts, flags and the probability column bit for bit,
    the cells those fixed-frame cells through the per-row f32 inverse matrices, bit for bit"""
    fixed, flags, counts = head.get_frame_occ(out['fused_roi_feats'], rois, res['local_xyz'], res['roi_inds'])
    assert counts == out['occ_counts'] and torch.equal(flags, out['occ_flags'])
    assert out['occ_ego'].shape == fixed.shape and torch.equal(fixed[:, 3], out['occ_ego'][:, 3])
    assert torch.equal(out['occ_ego'][:, :3], through(fixed, inv32, counts))
    return fixed, flags, counts


@pytest.fixture(scope='module')
def walk(dev, model):
    """both calls on every state, once: ``plain`` and ``occ`` through simple_test_scene_steps, ``ref`` and three twins
    through the existing operators and simple_test_steps(occ=True), the decoder logits of the reference call recorded"""
    rh = model.roi_head
    cfg = rh.SCENE_ROWS_DEFAULTS
    names = ('plain', 'occ', 'ref', 'twin0', 'twin1', 'twin2')
    states = {k: rh.online_begin(3, dev, cap=FRAMES) for k in names}
    frames, origin, calls, logits = head_frames(), {}, [], []
    decoder = rh.bbox_head.occ_ae_head.occ_decoder
    forward = decoder.forward

    def recording(*a, **k):
        out = forward(*a, **k)
        logits.append(out.detach().reshape(-1))
        return out

    for fs in CALLS:
        kw, m64, keys = call_inputs(dev, frames, fs, origin)
        rec = dict(kw=kw, m64=m64, keys=keys)
        rec['plain'] = rh.simple_test_scene_steps(**kw, state=states['plain'])
        with _StepsTap(rh.bbox_head) as tap:
            rec['occ'] = rh.simple_test_scene_steps(**kw, state=states['occ'], occ=True)
        rec['occ_rois'], rec['occ_res'] = tap.calls[-1]
        # ---- the reference: rows per frame with the existing operator, the boxes through the same matrices
        m_dev = torch.from_numpy(np.stack([m64[:, :3].reshape(-1, 12), np.linalg.inv(m64)[:, :3].reshape(-1, 12)])).to(dev)
        fixed = rh._boxes_through(kw['boxes'], m_dev[0])
        rec['inv32'] = m_dev[1].float()
        xyz, feats, row, counts = RS.per_frame_rows(
            kw['points'], kw['cloud_sizes'], kw['boxes'], kw['scores'], kw['frame_rows'], transforms=m_dev[0].float(), deco_boxes=fixed,
            extra_width=cfg['extra_width'], attr_dims=cfg['attr_dims'], point_cloud_range=cfg['point_cloud_range'],
            max_points=cfg['max_points'])
        rec['counts'] = counts
        for name in names[2:]:
            if name == 'ref':
                decoder.forward = recording
            try:
                rec[name] = rh.simple_test_steps(xyz, feats, row, fixed, kw['scores'], kw['labels'], kw['slot_rows'], states[name],
                                                 occ=True)
            finally:
                if name == 'ref':
                    del decoder.forward
        calls.append(rec)
    return dict(calls=calls, states=states, origin=origin, logits=torch.cat(logits), decoder=decoder, head=rh.bbox_head)


def _distances(walk, key, got):
    """(d0, distance): the largest distance of the three twin runs from the reference run, and of ``got`` from it, over
    both calls, relative to the reference's largest magnitude"""
    d0 = dist = 0.0
    for rec in walk['calls']:
        ref = rec['ref'][key].double()
        scale = float(ref.abs().max())
        d0 = max([d0] + [float((rec[t][key].double() - ref).abs().max()) / scale for t in ('twin0', 'twin1', 'twin2')])
        dist = max(dist, float((rec[got][key].double() - ref).abs().max()) / scale)
    return d0, dist


def test_two_calls_match_the_existing_operators(walk):
    """valid, num_points, state.frames and state.origin equal; boxes, scores and fused_roi_feats within 2 d0 + 1e-7
    relative, d0 the largest distance of three twin runs of the reference call from the first (the step is not
    bit-reproducible; the rule and the margin of the one-frame scene-step test)"""
    seen_invalid = False
    for rec, fs in zip(walk['calls'], CALLS):
        assert set(rec['plain']) == KEYS and set(rec['occ']) == KEYS | OCC_KEYS
        want_valid = [key != EMPTY for key in rec['keys']]
        seen_invalid = seen_invalid or not all(want_valid)
        for got in ('plain', 'occ'):
            out = rec[got]
            assert torch.equal(out['valid'], rec['ref']['valid']) and out['valid'].tolist() == want_valid
            assert torch.equal(out['num_points'], rec['counts']) and not out['num_points'].is_cuda
            assert [int(c) == 0 for c in out['num_points']] == [not v for v in want_valid]
    assert seen_invalid and [len(r['keys']) for r in walk['calls']] == [5, 3]
    assert walk['calls'][0]['kw']['slot_rows'] == [2, 2, 2, 0, 0] and walk['calls'][0]['kw']['frame_rows'] == [0, 1, 2, 1, 2]
    assert walk['calls'][1]['kw']['slot_rows'] == [2, 0, 0] and walk['calls'][1]['kw']['frame_rows'] == [0, 0, 1]
    states, origin = walk['states'], walk['origin']
    for got in ('plain', 'occ'):
        st = states[got]
        assert st.frames == [FRAMES, 0, FRAMES] == states['ref'].frames
        assert torch.equal(st.cache.pos, states['ref'].cache.pos)
        assert st.origin[1] is None and np.array_equal(st.origin[2], origin[0]) and np.array_equal(st.origin[0], origin[1])
    for got in ('plain', 'occ'):
        for key in CLOSE:
            d0, dist = _distances(walk, key, got)
            print(f'{got} {key}: twin runs of the reference d0 = {d0:.3e}, simple_test_scene_steps against the reference {dist:.3e}')
            assert dist <= 2 * d0 + 1e-7, (got, key, dist, d0)


def test_boxes_ego(walk):
    """valid rows within the bound of three f32 roundings of the float64 inverse map of the call's own refined box, the
    sizes kept and the yaw within an ulp of a yaw below 4; invalid rows keep their input box bit for bit"""
    seen_invalid = False
    for rec in walk['calls']:
        out, boxes = rec['occ'], rec['kw']['boxes']
        inv64 = np.linalg.inv(rec['m64'])[:, :3].reshape(-1, 12)
        got, refined = out['boxes_ego'].cpu().numpy(), out['boxes'].cpu().numpy()
        for r, ok in enumerate(out['valid'].tolist()):
            if not ok:
                seen_invalid = True
                assert torch.equal(out['boxes_ego'][r], boxes[r]) and torch.equal(rec['plain']['boxes_ego'][r], boxes[r])
                continue
            centre = R.transform64(refined[r:r + 1, :3], inv64[r])[0]
            assert (np.abs(got[r, :3] - centre) <= R.transform_bound(refined[r:r + 1, :3], inv64[r])[0]).all(), r
            assert np.array_equal(got[r, 3:6], refined[r, 3:6])
            yaw = refined[r, 6].astype(np.float64)
            hv = inv64[r].reshape(3, 4)[:2, :2] @ np.array([np.sin(yaw), np.cos(yaw)])
            turn = np.arctan2(hv[0], hv[1]) - got[r, 6]
            assert abs((turn + np.pi) % (2 * np.pi) - np.pi) <= 2.0 ** -22, r
    assert seen_invalid


def test_occ_of_every_row_in_its_own_ego_frame(walk):
    """occ=True: occ_counts and occ_flags equal the reference call's -- no decoder logit of the reference call lies within
    1e-3 of the threshold, asserted first --; the cells are the reference call's ``occ`` through the same f32 inverse
    matrices with the fill kernel's arithmetic, bit for bit.  The probability column is the sigmoid of the bf16 decoder's
    logit of a latent that differs from run to run (tests/test_gpu_online_occ.py), so it is asserted where it is exact: bit
    for bit against get_frame_occ on the call's OWN fused latents and pooled points, row by row (the rule of
    test_scene_step_occ_ego_goes_back_to_the_fixed_frame_cells there); its distance from the reference's and the twin
    runs' is printed.  With MODEL_SEED every cell is predicted, so counts and bit 0 of the flags do not discriminate here:
    the selection is exercised by test_occ_selection_of_a_model_whose_logits_straddle_the_threshold."""
    decoder = walk['decoder']
    margin = float((walk['logits'] - math.log(decoder.pos_thresh / (1 - decoder.pos_thresh))).abs().min())
    print(f'{walk["logits"].numel()} decoder logits, the nearest {margin:.3e} from the threshold')
    assert margin >= 1e-3, 'precondition on the input: change MODEL_SEED'
    d0 = dist = 0.0
    cells = 0
    for rec in walk['calls']:
        out, ref = rec['occ'], rec['ref']
        assert out['occ_counts'] == ref['occ_counts'] and torch.equal(out['occ_flags'], ref['occ_flags'])
        assert out['occ_ego'].shape == (sum(out['occ_counts']), 4) and out['occ_ego'].dtype == torch.float32
        assert all(c > 0 for key, c in zip(rec['keys'], out['occ_counts']) if key != EMPTY)      # (a row with points has cells)
        assert torch.equal(out['occ_ego'][:, :3], through(ref['occ'], rec['inv32'], ref['occ_counts']))
        assert bool(((out['occ_ego'][:, 3] > decoder.pos_thresh) == ((out['occ_flags'] & 1) != 0)).all())
        assert_occ_of_own_latents(walk['head'], out, rec['occ_rois'], rec['occ_res'], rec['inv32'])
        assert float(out['occ_ego'][:, 3].max() - out['occ_ego'][:, 3].min()) > 0.05        # (not one value for all cells)
        for t in ('twin0', 'twin1', 'twin2'):
            assert rec[t]['occ_counts'] == ref['occ_counts']
            d0 = max(d0, float((rec[t]['occ'][:, 3].double() - ref['occ'][:, 3].double()).abs().max()))
        dist = max(dist, float((out['occ_ego'][:, 3].double() - ref['occ'][:, 3].double()).abs().max()))
        cells += sum(out['occ_counts'])
    print(f'{cells} cells; probability column: twin runs d0 = {d0:.3e}, simple_test_scene_steps against the reference {dist:.3e}')
    assert cells > 100


def test_occ_selection_of_a_model_whose_logits_straddle_the_threshold(dev):
    """the same two calls with occ=True on a model (seed 0) that decodes some cells as occupied and most not -- the
    precondition of the test above cannot hold for such a model, so nothing is compared across runs: counts, flags,
    probabilities and cells are those of get_frame_occ on each call's own latents and pooled points, bit for bit; predicted
    and unpredicted, observed and unobserved cells all occur, and the row without a point has no observed cell"""
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (register)
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    torch.manual_seed(0)
    rh = DETECTORS.build(ococcnet_model_cfg()).to(dev).eval().roi_head
    state, frames, origin = rh.online_begin(3, dev, cap=FRAMES), head_frames(), {}
    total = pred = seen = 0
    for fs in CALLS:
        kw, m64, keys = call_inputs(dev, frames, fs, origin)
        with _StepsTap(rh.bbox_head) as tap:
            out = rh.simple_test_scene_steps(**kw, state=state, occ=True)
        rois, res = tap.calls[-1]
        inv32 = torch.from_numpy(np.linalg.inv(m64)[:, :3].reshape(-1, 12)).to(dev).float()
        _, flags, counts = assert_occ_of_own_latents(rh.bbox_head, out, rois, res, inv32)
        cuts = np.cumsum([0] + counts)
        for r, key in enumerate(keys):
            mine = flags[cuts[r]:cuts[r + 1]]
            assert (int(((mine & 2) != 0).sum()) == 0) == (key == EMPTY), key
        total, pred, seen = total + len(flags), pred + int(((flags & 1) != 0).sum()), seen + int(((flags & 2) != 0).sum())
    print(f'{total} cells kept, {pred} predicted, {seen} observed')
    assert 100 < pred < total and 100 < seen < total and state.frames == [FRAMES, 0, FRAMES]


def test_refusals_leave_the_state_alone(dev, model):
    rh = model.roi_head
    frames, origin = head_frames(), {}
    state = rh.online_begin(3, dev, cap=FRAMES)
    kw, _, _ = call_inputs(dev, frames, CALLS[0], origin)
    snapshot = lambda: (list(state.frames), state.cache.pos.clone(), [None if o is None else o.copy() for o in state.origin],
                        [k.clone() for k in state.cache.k])

    def unchanged(before):
        now = snapshot()
        return (now[0] == before[0] and torch.equal(now[1], before[1]) and all(torch.equal(a, b) for a, b in zip(now[3], before[3]))
                and all((a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))
                        for a, b in zip(now[2], before[2])))

    before = snapshot()
    with pytest.raises(L.OcoccError, match='strictly increasing'):          # slot 2's run goes back in time
        rh.simple_test_scene_steps(**dict(kw, frame_rows=[0, 2, 1, 1, 2]), state=state)
    with pytest.raises(L.OcoccError, match='strictly increasing'):          # slot 0's run repeats a cloud
        rh.simple_test_scene_steps(**dict(kw, frame_rows=[0, 1, 2, 1, 1]), state=state)
    assert unchanged(before)
    empty = rh.simple_test_scene_steps(kw['points'], kw['cloud_sizes'], kw['poses'], kw['boxes'][:0], kw['scores'][:0], kw['labels'][:0],
                                       [], [], state, occ=True)
    assert set(empty) == KEYS | OCC_KEYS and all(len(v) == 0 for v in empty.values()) and unchanged(before)
    assert empty['boxes_ego'].shape == (0, 7) and empty['occ_ego'].shape == (0, 4) and empty['occ_counts'] == []
    # a slot in mid-tracklet without an origin: stepped through simple_test_steps, whose caller keeps the fixed frame
    rh.simple_test_scene_steps(**kw, state=state)
    assert state.frames == [2, 0, 3] and state.origin[1] is None
    state.origin[0] = None
    before = snapshot()
    nxt, _, _ = call_inputs(dev, frames, CALLS[1], origin)
    with pytest.raises(L.OcoccError, match='no origin'):
        rh.simple_test_scene_steps(**nxt, state=state)
    assert unchanged(before)


def test_replay_in_chunks_of_three(dev, model, tmp_path):
    """make_synthetic_raw's tree (1 segment, 2 objects and a false positive above every point, 6 frames) replayed with
    chunk = 3 and chunk = 1: the same records in the same order -- ids, timestamps, num_points and refined equal, unrefined
    objects the tracker's box and score bit for bit, all boxes finite --, every slot released, --slots too small still an
    error, and with save_occ one file per refined (object, frame), the files chunk = 1 writes"""
    import importlib.util
    from objectcentricocccompletion_amd import occ_export, waymo_io
    tools = os.path.join(ROOT, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import make_synthetic_raw
    spec = importlib.util.spec_from_file_location('ococc_tools_online_raw', os.path.join(tools, 'online_raw.py'))
    online_raw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(online_raw)
    root = str(tmp_path / 'raw')
    make_synthetic_raw.main([root, '--segments', '1', '--tracklets', '2', '--frames', '6', '--background', '500'])
    yaml, poses = os.path.join(root, 'synthetic_vehicle.yaml'), os.path.join(root, 'poses.pkl')
    one, state1 = online_raw.replay(model, yaml, slots=4, poses=poses, save_occ=str(tmp_path / 'occ1'))
    out = str(tmp_path / 'chunked.bin')
    got, state = online_raw.replay(model, yaml, slots=4, poses=poses, out=out, chunk=3, save_occ=str(tmp_path / 'occ3'))
    assert state.frames == [0, 0, 0, 0] and state.origin == [None] * 4 and state.cache.cap == 6
    assert len(got) == len(one) >= 12 and [list(r) for r in got] == [list(r) for r in one]
    tracker = {(t.segment_name, t.id): t for t in waymo_io.generate_tracklets(waymo_io.read_bin(os.path.join(root, 'waymo_format', 'pred.bin')))}
    for a, b in zip(got, one):
        assert all(a[k] == b[k] for k in ('segment', 'id', 'type', 'timestamp', 'num_points', 'refined'))
        assert np.isfinite(a['box']).all() and a['box'].shape == (7,) and math.isfinite(a['score'])
        if not a['refined']:
            t = tracker[(a['segment'], a['id'])]
            i = t.ts2index[a['timestamp']]
            assert np.array_equal(a['box'], t.boxes[i].numpy()) and a['score'] == float(t.scores[i])
    assert sum(r['refined'] for r in got) >= 6 and sum(not r['refined'] for r in got) >= 6
    assert len(waymo_io.read_bin(out)) == len(got)
    listing = lambda d: sorted(os.path.relpath(os.path.join(p, n), d) for p, _, names in os.walk(d) for n in names)
    assert listing(str(tmp_path / 'occ3')) == listing(str(tmp_path / 'occ1'))
    for r in got:
        if r['refined']:
            cells = occ_export.read_occ_bin(occ_export.occ_path(str(tmp_path / 'occ3'), r['segment'], r['timestamp'], r['type'], r['id']))
            assert cells.shape == (r['occ_cells'], 4) and r['occ_cells'] > 0 and (cells[:, 3] == np.float32(r['score'])).all()
    with pytest.raises(L.OcoccError, match='--slots'):
        online_raw.replay(model, yaml, slots=2, poses=poses, chunk=3)
