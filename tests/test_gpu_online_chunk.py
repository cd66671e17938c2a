"""Online inference with several frames per tracklet in one call (occ/layers.py: TemporalCache.check_steps, *.steps;
OccBBoxHead.forward_steps; TrackletRoIHeadOCC.simple_test_steps; test_cfg.online_chunk) against the offline pass over the
whole tracklet.  The attention of a chunk is bit for bit that of the single steps (tests/test_gpu_attention_chunk.py); what
is left between a chunked pass and the offline pass is f32 arithmetic at other GEMM row counts, which both tests below
measure on existing code first, as tests/test_gpu_online.py does, and hold the chunked path to twice of it.  The float64
restatement of the encoder layer, the tracklet synthesiser (same seed) and the tap restate those of that file."""
import math

import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu


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


def _future_mask(L, window, dev):
    """OccBBoxHead.get_future_mask: True = may not attend"""
    mask = torch.triu(torch.ones(L, L, dtype=torch.bool, device=dev), diagonal=1)
    if window > 0:
        for i in range(window - 1, L):
            mask[i, :i - window + 1] = True
    return mask


def _layer64(layer, x, pos, mask):
    """SimpleEncoderLayer restated in plain float64 torch on the host: q = k = x + pos, v = x, post-LN, the layer's activation"""
    F = torch.nn.functional
    p = lambda t: t.detach().double().cpu()
    att = layer.self_attn
    E, H = att.embed_dim, att.num_heads
    D = E // H
    w, b = p(att.in_proj_weight), p(att.in_proj_bias)
    qk_in = x + pos
    q, k, v = qk_in @ w[:E].t() + b[:E], qk_in @ w[E:2 * E].t() + b[E:2 * E], x @ w[2 * E:].t() + b[2 * E:]
    L = x.shape[0]
    scores = torch.einsum('lhd,shd->hls', q.view(L, H, D) * D ** -0.5, k.view(L, H, D))
    scores = scores.masked_fill(mask.cpu()[None], float('-inf'))
    ctx = torch.einsum('hls,shd->lhd', torch.softmax(scores, -1), v.view(L, H, D)).reshape(L, E)
    attended = ctx @ p(att.out_proj.weight).t() + p(att.out_proj.bias)
    x = F.layer_norm(x + attended, (E,), p(layer.norm1.weight), p(layer.norm1.bias), layer.norm1.eps)
    ff = layer.activation(x @ p(layer.linear1.weight).t() + p(layer.linear1.bias)) @ p(layer.linear2.weight).t() \
        + p(layer.linear2.bias)
    return F.layer_norm(x + ff, (E,), p(layer.norm2.weight), p(layer.norm2.bias), layer.norm2.eps)


def _dist(a, ref):
    return float((a.double().cpu() - ref.double().cpu()).abs().max() / ref.double().abs().max())


@pytest.mark.parametrize('window', [-1, 3])
def test_encoder_chunks_match_the_masked_forward(dev, window):
    """The stack of test_encoder_steps_match_the_masked_forward: 3 layers, d_model 64, 4 heads, ffn 32; two tracklets of 6
    and 4 frames in slots 2 and 0 of a three-slot cache.  Two ``steps`` calls with unequal runs -- slot 2 frames 0-3 plus
    slot 0 frame 0, then slot 2 frames 4-5 plus slot 0 frames 1-3 -- and, with the window, the same calls through a ring
    of cap = window = 3 rows, whose first run of 4 overwrites its own frame 0.  The chunked rows may be twice as far from
    float64 as the offline pass is: the existing rule."""
    from objectcentricocccompletion_amd.occ.layers import (PositionalEncoding, SimpleEncoderLayer, TemporalCache,
                                                           TransformerEncoder)
    torch.manual_seed(5)
    E, lens, slot_of = 64, [6, 4], [2, 0]
    enc = TransformerEncoder(SimpleEncoderLayer(E, 4, dim_feedforward=32, dropout=0.1), 3)
    with torch.no_grad():
        for prm in enc.parameters():   # (the clones start identical, the biases at zero)
            prm.copy_(torch.randn_like(prm) * prm.shape[1] ** -0.5 if prm.dim() == 2 else prm + 0.1 * torch.randn_like(prm))
    enc = enc.to(dev).eval()
    src = [torch.randn(n, E) for n in lens]
    pe = [PositionalEncoding(E)(torch.arange(n)) + 0.5 * torch.randn(n, E) for n in lens]
    off, ref = [], []
    with torch.no_grad():
        for x, p in zip(src, pe):
            mask = _future_mask(x.shape[0], window, dev)
            off.append(enc(x.to(dev)[:, None], pos_enc=p.to(dev)[:, None], attn_mask=mask)[:, 0])
            y = x.double()
            for layer in enc.layers:
                y = _layer64(layer, y, p.double(), mask)
            ref.append(y)
    off, ref = torch.cat(off), torch.cat(ref)
    e_off = _dist(off, ref)
    calls = [[(0, 0, 4), (1, 0, 1)], [(0, 4, 6), (1, 1, 4)]]                 # (tracklet, first frame, end) per call
    caches = [TemporalCache(3, 3, E, dev, cap=8)] + ([TemporalCache(3, 3, E, dev, cap=3, ring=True)] if window > 0 else [])
    for cache in caches:
        got = [[] for _ in lens]
        for call in calls:
            rows = [(b, t) for b, lo, hi in call for t in range(lo, hi)]
            out = enc.steps(torch.stack([src[b][t] for b, t in rows]).to(dev), torch.stack([pe[b][t] for b, t in rows]).to(dev),
                            [slot_of[b] for b, _ in rows], cache, window)
            for i, (b, _) in enumerate(rows):
                got[b].append(out[i])
        assert cache.pos_host == [4, 0, 6] and cache.pos.tolist() == [4, 0, 6]
        e_chunk = _dist(torch.cat([torch.stack(g) for g in got]), ref)
        print(f'encoder stack, window {window}, ring {cache.ring}: offline against float64 {e_off:.3e}, chunks against '
              f'float64 {e_chunk:.3e}')
        assert e_chunk <= 2 * e_off + 1e-7, (e_chunk, e_off)
    with pytest.raises(RuntimeError):
        enc.train().steps(src[0][:1].to(dev), pe[0][:1].to(dev), [1], caches[0], window)


# ---------------------------------------------------------------------------------------------------------------------
L_FRAMES, EMPTY_FRAME, SEED, CHUNK = 8, 6, 6, 3


def _tracklet_inputs(dev, upto=L_FRAMES):
    """Tracklet 1 of synth_tracklets(2, 8, 90): its frame 6 comes without points; here it gets 20 points 40 m away from
    its box, so the frame has points and none of them in the box.  ``upto``: the prefix of that many frames, the same
    coordinates."""
    from objectcentricocccompletion_amd.tracklet import Tracklet
    t = synth.synth_tracklets(2, L_FRAMES, 90, seed=SEED)
    rng = np.random.default_rng(SEED)
    rb = t['rois'][t['rois'][:, 0] == 1][:, 1:]
    m = t['pts_batch'] == 1
    score = rng.uniform(0.3, 1.0, size=L_FRAMES).astype(np.float32)
    fr, xyz, attr = t['pts_frame'][m], t['pts_xyz'][m], t['pts_attr'][m]
    assert not (fr == EMPTY_FRAME).any() and all((fr == f).any() for f in range(L_FRAMES) if f != EMPTY_FRAME)
    stray = np.flatnonzero(fr == EMPTY_FRAME - 1)[:20]
    xyz = np.concatenate([xyz, xyz[stray] + np.array([40, 0, 0], np.float32)])
    attr, fr = np.concatenate([attr, attr[stray]]), np.concatenate([fr, np.full(len(stray), EMPTY_FRAME)])
    deco = np.concatenate([attr, rb[fr][:, 6:7] / np.pi, rb[fr][:, 3:6] / 10, score[fr][:, None]], 1)
    pts = np.concatenate([xyz, deco], 1).astype(np.float32)
    gt = rb + rng.normal(0, [0.1, 0.1, 0.05, 0.05, 0.05, 0.05, 0.02], rb.shape).astype(np.float32)
    far = gt.copy()
    far[:, :2] += 30
    occ = np.concatenate([(rng.random((24, 3)) - 0.5) * [4.5, 2.0, 1.6], rng.integers(0, 3, (24, 1))], 1).astype(np.float32)
    keep = fr < upto
    ts = list(range(1100, 1100 + upto))
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(points=[T(pts[keep])], pts_frame_inds=[T(fr[keep])], img_metas=None,
                tracklet=[Tracklet(T(rb[:upto]), ts, T(score[:upto]), type=0)],
                gt_tracklet_candidates=[[Tracklet(T(far[:upto]), ts, type=0), Tracklet(T(gt[:upto]), ts, type=0)]],
                occ_labels=[[T(occ)] * 2], occ_labels_scores=[[torch.tensor([0.9], device=dev)] * 2])


class _Tap(object):
    """records what a test run decodes (boxes, scores, valid mask), the shape latents its occupancy counts are made from
    and the decoder logits behind those counts -- through the public methods both paths call -- and the slot lists of the
    simple_test_step / simple_test_steps calls it makes"""

    def __init__(self, rh):
        self.rh, self.decoded, self.feats, self.logits, self.step_calls, self.steps_calls = rh, [], [], [], [], []

    def __enter__(self):
        head, rh = self.rh.bbox_head, self.rh
        get, occ, step, steps = head.get_bboxes_from_tracklet, rh.test_occ, rh.simple_test_step, rh.simple_test_steps

        def get_bboxes(*a, **k):
            out = get(*a, **k)
            self.decoded.append(out[0])
            return out

        def test_occ(rois, feats, *a, **k):
            self.feats.append(feats)
            return occ(rois, feats, *a, **k)

        def simple_test_step(pts_xyz, pts_feats, pts_batch_idx, boxes, scores, labels, slot, state, **k):
            self.step_calls.append(list(slot))
            return step(pts_xyz, pts_feats, pts_batch_idx, boxes, scores, labels, slot, state, **k)

        def simple_test_steps(pts_xyz, pts_feats, pts_row_idx, boxes, scores, labels, slot_rows, state, **k):
            self.steps_calls.append(list(slot_rows))
            return steps(pts_xyz, pts_feats, pts_row_idx, boxes, scores, labels, slot_rows, state, **k)

        head.get_bboxes_from_tracklet, rh.test_occ = get_bboxes, test_occ
        rh.simple_test_step, rh.simple_test_steps = simple_test_step, simple_test_steps
        self.hook = head.occ_ae_head.occ_decoder.register_forward_hook(lambda m, i, o: self.logits.append(o.detach()))
        return self

    def __exit__(self, *exc):
        del self.rh.bbox_head.get_bboxes_from_tracklet, self.rh.test_occ, self.rh.simple_test_step, self.rh.simple_test_steps
        self.hook.remove()

    def result(self):
        cat = lambda j: torch.cat([d[j] for d in self.decoded], 0)
        return dict(boxes=cat(0), scores=cat(1), valid=cat(3), fused_roi_feats=torch.cat(self.feats, 0))


def _simple_test(model, dev):
    kw = _tracklet_inputs(dev)
    xyz, feats, batch, frames = model._cat_points(kw['points'], kw['pts_frame_inds'])
    return model.roi_head.simple_test(
        pts_xyz=xyz, pts_feats=feats, pts_batch_idx=batch, pts_frame_inds=frames, img_metas=None,
        tracklet_list=kw['tracklet'], gt_candidates_list=kw['gt_tracklet_candidates'],
        gt_occs_list=kw['occ_labels'], gt_occ_scores_list=kw['occ_labels_scores'])[0]


@pytest.fixture(scope='module')
def runs(dev):
    """the ococcnet model on one tracklet of 8 frames: the offline pass over the whole tracklet and over every prefix, the
    online pass in chunks of 3 frames and the one under online_chunk = 1 -- computed once for the tests below.  The
    offline pass is not bit-reproducible from run to run, so every prefix is run three times and d0 is the
    largest distance over all of them: one pass over the prefixes gave d0 = 3.6e-07, 5.0e-07 and 6.6e-07 for the boxes in
    three runs of this file and two passes 4.3e-07 in a fourth, while the online figure it bounds was 8.571e-07 in all
    of them, single steps and chunks alike -- a yardstick taken from one pass fails the unchanged code every few runs."""
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (register)
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    torch.manual_seed(0)
    model = DETECTORS.build(ococcnet_model_cfg()).to(dev).eval()
    rh = model.roi_head
    assert not rh.test_cfg.get('online', False) and rh.test_cfg.get('test_occ_iou', False)
    assert 'online_chunk' not in rh.test_cfg
    out = dict(model=model, prefix=[])
    with torch.no_grad():
        with _Tap(rh) as tap:
            out['offline_result'] = model(return_loss=False, **_tracklet_inputs(dev))[0]
        out['offline'], out['offline_logits'] = tap.result(), torch.cat([l.view(-1) for l in tap.logits])
        for upto in list(range(1, L_FRAMES + 1)) * 3:
            with _Tap(rh) as tap:
                model(return_loss=False, **_tracklet_inputs(dev, upto))
            out['prefix'].append(tap.result())
        rh.test_cfg['online'] = True
        try:
            for key, chunk in (('chunk', CHUNK), ('one', 1)):
                rh.test_cfg['online_chunk'] = chunk
                with _Tap(rh) as tap:
                    out[key + '_result'] = _simple_test(model, dev)
                out[key], out[key + '_calls'] = tap.result(), (tap.step_calls, tap.steps_calls)
        finally:
            rh.test_cfg['online'] = False
            rh.test_cfg.pop('online_chunk', None)
    return out


def _d0(runs, key):
    """the largest distance between row t of the full offline pass and the last row of an offline pass over frames 0..t"""
    full = runs['offline'][key].double()
    scale = float(full.abs().max())
    return max(float((run[key][-1].double() - full[run[key].shape[0] - 1]).abs().max()) / scale for run in runs['prefix']), scale


def _assert_online_matches_offline(runs, on, result):
    """the rule of tests/test_gpu_online.py for one online pass: ``on`` what it decoded, ``result`` what simple_test returned"""
    off = runs['offline']
    assert torch.equal(on['valid'], off['valid'])
    for key in ('boxes', 'scores', 'fused_roi_feats'):
        full = off[key].double()
        d0, scale = _d0(runs, key)
        d_on = max(float((on[key][t].double() - full[t]).abs().max()) / scale for t in range(L_FRAMES))
        print(f'{key}: prefix runs against the full run d0 = {d0:.3e}, online in chunks against the full run {d_on:.3e}')
        assert d_on <= 2 * d0 + 1e-7, (key, d_on, d0)
    a = runs['offline_result']
    assert len(a['inters']) > 0 and int(torch.cat(a['unions']).sum()) > 0
    assert torch.equal(torch.cat(a['inters']), torch.cat(result['inters']))
    assert torch.equal(torch.cat(a['unions']), torch.cat(result['unions']))
    assert torch.equal(torch.cat(a['gt_boxes']), torch.cat(result['gt_boxes']))
    ta, tb = a['out_tracklets'][0], result['out_tracklets'][0]
    assert ta.boxes.shape == tb.boxes.shape == (L_FRAMES, 7)
    assert torch.equal(ta.boxes[EMPTY_FRAME], tb.boxes[EMPTY_FRAME])      # the RoI without points keeps its proposal
    valid = off['valid']
    assert torch.equal(tb.boxes[valid], on['boxes'][valid])               # ... and the others are the decoded boxes


def test_whole_model_in_chunks_matches_offline(runs):
    """test_cfg.online_chunk = 3 through simple_test: the calls take the frames 0-2, 3-5 and 6-7 (frame 6 has no point in
    its box).  Boxes, scores and the fused shape latents lie within 2 d0 + 1e-7 of the full offline pass, d0 measured on
    the offline prefixes; the valid mask and the occupancy counts per RoI are equal -- no offline decoder logit of this
    input is within 1e-3 of the decision threshold, asserted first."""
    decoder = runs['model'].roi_head.bbox_head.occ_ae_head.occ_decoder
    margin = float((runs['offline_logits'] - math.log(decoder.pos_thresh / (1 - decoder.pos_thresh))).abs().min())
    print(f'{runs["offline_logits"].numel()} decoder logits, the nearest {margin:.3e} from the threshold')
    assert margin >= 1e-3, 'precondition on the input: change SEED'
    assert runs['offline']['valid'].tolist() == [f != EMPTY_FRAME for f in range(L_FRAMES)]
    assert runs['chunk_calls'] == ([], [[0] * 3, [0] * 3, [0] * 2])
    _assert_online_matches_offline(runs, runs['chunk'], runs['chunk_result'])


def test_online_chunk_of_one_makes_the_single_step_calls(runs):
    """online_chunk = 1 is today's path: one simple_test_step call per frame, no simple_test_steps call, the same rule"""
    assert runs['one_calls'] == ([[0]] * L_FRAMES, [])
    _assert_online_matches_offline(runs, runs['one'], runs['one_result'])


def test_steps_of_two_tracklets_at_different_frame_counts(runs, dev):
    """simple_test_steps with the rows of two tracklets in one call: slot 0 has been stepped through 3 frames and takes the
    frames 3-5, slot 1 is new and takes the frames 0-4 (both follow the tracklet of the tests above).  Every row agrees with
    the single step of its frame (online_chunk = 1 above) and with the full offline pass by the rule of those tests; the
    valid flags are equal."""
    model = runs['model']
    rh = model.roi_head
    kw = _tracklet_inputs(dev)
    xyz, feats, _, frames = model._cat_points(kw['points'], kw['pts_frame_inds'])
    trk = kw['tracklet'][0]
    rois, _, scores, labels = rh.tracklets2rois([trk])

    def call(state, rows):
        """rows: (slot, frame) pairs"""
        sel = [torch.nonzero(frames == f)[:, 0] for _, f in rows]
        fr = torch.tensor([f for _, f in rows], device=dev)
        row_idx = torch.cat([torch.full_like(s, i) for i, s in enumerate(sel)])
        sel = torch.cat(sel)
        return rh.simple_test_steps(xyz[sel], feats[sel], row_idx, rois[fr, 1:8], scores[fr], labels[fr],
                                    [s for s, _ in rows], state)

    state = rh.online_begin(2, dev, cap=L_FRAMES)
    with torch.no_grad():
        call(state, [(0, 0), (0, 1), (0, 2)])
        assert state.frames == [3, 0]
        rows = [(1, f) for f in range(5)] + [(0, f) for f in range(3, 6)]
        res = call(state, rows)
    assert state.frames == [6, 5] and state.cache.pos.tolist() == [6, 5]
    fr = [f for _, f in rows]
    assert torch.equal(res['valid'], runs['one']['valid'][fr]) and bool(res['valid'].all())
    for key in ('boxes', 'scores', 'fused_roi_feats'):
        d0, scale = _d0(runs, key)
        for name, other in (('single steps', runs['one']), ('offline pass', runs['offline'])):
            d = float((res[key].double() - other[key][fr].double()).abs().max()) / scale
            print(f'{key}: rows of two tracklets against the {name} {d:.3e} (d0 = {d0:.3e})')
            assert d <= 2 * d0 + 1e-7, (key, name, d, d0)


@pytest.mark.parametrize('ring', [False, True])
def test_encoder_steps_of_one_frame_are_the_step(dev, ring):
    """``steps`` with a run of one frame per slot against ``step`` on twin caches: the two share everything but the
    attention export, whose chunk mode computes the step's sums in the step's order, so the output, every layer's keys and
    values, ``pos`` and ``pos_host`` are equal bit for bit.  2 layers, E = 32, 2 heads, ffn 64; rows for the slots [2, 0]
    of a three-slot cache that holds 1, 0 and 3 frames (cap 4), and of a ring of cap = window = 3 at frames 7, 0 and 4,
    where both new rows overwrite an old frame."""
    from objectcentricocccompletion_amd.occ.layers import SimpleEncoderLayer, TemporalCache, TransformerEncoder
    torch.manual_seed(11)
    E, slots = 32, [2, 0]
    enc = TransformerEncoder(SimpleEncoderLayer(E, 2, dim_feedforward=64, dropout=0.1), 2)
    with torch.no_grad():
        for prm in enc.parameters():
            prm.copy_(torch.randn_like(prm) * prm.shape[1] ** -0.5 if prm.dim() == 2 else prm + 0.1 * torch.randn_like(prm))
    enc = enc.to(dev).eval()
    kw, window, pos = (dict(cap=3, ring=True), 3, [7, 0, 4]) if ring else (dict(cap=4), -1, [1, 0, 3])
    twins = [TemporalCache(2, 3, E, dev, **kw) for _ in range(2)]
    rows = [torch.randn_like(k) for k in twins[0].k + twins[0].v]
    for cache in twins:
        for t, r in zip(cache.k + cache.v, rows):
            t.copy_(r)
        cache.pos.copy_(torch.tensor(pos, dtype=torch.int32))
        cache.pos_host = list(pos)
    src, pe = torch.randn(2, E, device=dev), torch.randn(2, E, device=dev)
    one = enc.step(src, pe, slots, twins[0], window)
    many = enc.steps(src, pe, slots, twins[1], window)
    assert torch.equal(one, many) and bool(torch.isfinite(one).all())
    for a, b, r in zip(twins[0].k + twins[0].v, twins[1].k + twins[1].v, rows):
        assert torch.equal(a, b) and not torch.equal(a, r)
    after = [p + (s in slots) for s, p in enumerate(pos)]
    for cache in twins:
        assert cache.pos_host == after and cache.pos.tolist() == after


def test_three_steps_and_one_chunk_of_three_leave_the_same_state(runs, dev):
    """frames 0-2 of the tracklet above with ``occ=True``, as three simple_test_step calls and as one simple_test_steps
    call with a run of three: the frame counters on the host and on the device are equal, both forms return the same nine
    keys, the valid flags are equal and boxes, scores and fused latents agree by the rule of the tests above."""
    model = runs['model']
    rh = model.roi_head
    kw = _tracklet_inputs(dev)
    xyz, feats, _, frames = model._cat_points(kw['points'], kw['pts_frame_inds'])
    rois, _, scores, labels = rh.tracklets2rois(kw['tracklet'])
    sel = [torch.nonzero(frames == f)[:, 0] for f in range(3)]
    single, chunked = rh.online_begin(1, dev, cap=L_FRAMES), rh.online_begin(1, dev, cap=L_FRAMES)
    with torch.no_grad():
        steps = [rh.simple_test_step(xyz[s], feats[s], torch.zeros_like(s), rois[f:f + 1, 1:8], scores[f:f + 1],
                                     labels[f:f + 1], [0], single, occ=True) for f, s in enumerate(sel)]
        chunk = rh.simple_test_steps(xyz[torch.cat(sel)], feats[torch.cat(sel)],
                                     torch.cat([torch.full_like(s, f) for f, s in enumerate(sel)]), rois[:3, 1:8], scores[:3],
                                     labels[:3], [0] * 3, chunked, occ=True)
    assert single.cache.pos_host == chunked.cache.pos_host == [3] and single.frames == chunked.frames
    assert single.cache.pos.tolist() == chunked.cache.pos.tolist() == [3]
    keys = {'boxes', 'scores', 'labels', 'valid', 'fused_roi_feats', 'ori_roi_feats', 'occ', 'occ_flags', 'occ_counts'}
    assert set(chunk) == keys and all(set(s) == keys for s in steps)
    assert len(chunk['occ_counts']) == 3 and all(len(s['occ_counts']) == 1 for s in steps)
    assert torch.equal(chunk['valid'], torch.cat([s['valid'] for s in steps])) and bool(chunk['valid'].all())
    for key in ('boxes', 'scores', 'fused_roi_feats'):
        d0, scale = _d0(runs, key)
        d = float((chunk[key].double() - torch.cat([s[key] for s in steps]).double()).abs().max()) / scale
        print(f'{key}: one chunk of three against three single steps {d:.3e} (d0 = {d0:.3e})')
        assert d <= 2 * d0 + 1e-7, (key, d, d0)
