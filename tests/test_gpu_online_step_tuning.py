"""Tuning per online step on the MI355X: OccBBoxHead.forward_step / forward_steps with ``tune=`` on the head
and the 2 tracklets x 3 frames of tests/test_gpu_online_tuning.py, the independence of a RoI's first gradient from its
company, and the tuned steps end to end (simple_test_step with ``occ``, simple_test under test_cfg.online_step_tuning,
tools/online_raw.py --step-tuning).

The point encoders sum with float atomics, so two passes of ``_encode_rois`` agree to rounding only.  What is
compared bit for bit between two runs here is everything BEHIND the encoders: their outputs are computed once per set of
rows and replayed, so a run that tunes and a run that never tuned see the same encoder outputs."""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_tune_ref as R                                                            # noqa: E402
import tune_sample_ref as ref                                                          # noqa: E402
from test_gpu_online_tuning import EMPTY, PICK, _leave_the_generators_alone, head, inputs   # noqa: E402,F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'ococcnet_mi355x.py')
TUNE = dict(num_iter=5, downsample_size=64, balance_sample=True, seed=0)
KEYS = ('fused_roi_feats', 'ori_roi_feats', 'cls_score', 'bbox_pred', 'nonempty_roi_mask')
SLOTS = [0, 1]


class _Replay(object):
    """``_encode_rois`` computed once per ``key`` and handed out again"""

    def __init__(self, real):
        self.real, self.store, self.key = real, {}, None

    def __call__(self, *a):
        if self.key not in self.store:
            self.store[self.key] = self.real(*a)
        return self.store[self.key]


@pytest.fixture(scope='module')
def replay(head):
    r = _Replay(head._encode_rois)
    head._encode_rois = r
    yield r
    del head._encode_rois


def _rows(inputs, rows, dev):
    """the rows ``rows`` of the six RoIs as a step takes them: column 0 of a roi its own index"""
    pts_xyz, pts_feats, info, roi_inds, rois, frames = inputs
    new = torch.full((len(PICK),), -1, dtype=torch.long, device=dev)
    new[rows] = torch.arange(len(rows), device=dev)
    sel = new[roi_inds] >= 0
    r = rois[rows].clone()
    r[:, 0] = torch.arange(len(rows), device=dev)
    return (pts_xyz[sel], pts_feats[sel], {k: v[sel] for k, v in info.items()}, new[roi_inds][sel], r, frames[rows])


def _cache(head, dev):
    from objectcentricocccompletion_amd.occ.layers import TemporalCache
    return TemporalCache(head.trans_enc.num_layers, 2, head.roi_feature_channels, dev, cap=4)


def _walk(head, replay, inputs, dev, steps, tune_at=()):
    """frames 0 .. steps - 1 of the two tracklets through forward_step, tuned at the frames ``tune_at``"""
    cache, outs = _cache(head, dev), []
    for t in range(steps):
        rows = [t, 3 + t]
        replay.key = tuple(rows)
        outs.append(head.forward_step(*_rows(inputs, rows, dev), SLOTS, cache, return_points=True,
                                      tune=dict(TUNE) if t in tune_at else None))
    torch.cuda.synchronize()
    return outs, cache


def _sample(head, res, rois, frame):
    """the sample of a step's rows, drawn by the test: occ_ops.tune_sample on the step's own points"""
    from objectcentricocccompletion_amd.occ import occ_ops
    from objectcentricocccompletion_amd.tracklet import host_index
    ae = head.occ_ae_head
    sizes, dims, start, total = occ_ops.dense_grid_layout(rois[:, 4:7], ae.voxel_size, ae.scale_wlh, ae.offset_wlh)
    seeds = [ref.row_seed(TUNE['seed'], s, frame) for s in SLOTS]
    args = (sizes, dims, start, total, ae.voxel_size, ae.observation_xyz(res['local_xyz']), res['roi_inds'],
            host_index(seeds, rois.device), res['nonempty_roi_mask'])
    got = occ_ops.tune_sample(*args, balance=True, cap=TUNE['downsample_size'])
    exp = ref.tune_sample_ref(sizes.cpu().numpy(), dims.cpu().numpy(), start.cpu().numpy(), total, ae.voxel_size,
                              args[5].cpu().numpy(), args[6].cpu().numpy(), seeds, args[8].cpu().numpy(), True,
                              TUNE['downsample_size'])
    assert got[4] == exp[4] and all(g.cpu().numpy().tobytes() == e.tobytes() for g, e in zip(got[:4], exp[:4]))
    return got


def _bce_per_roi(head, latent, xyz, labels, index):
    with torch.no_grad():
        logits = head.occ_ae_head.decode(latent, xyz, index.long()).view(-1).double()
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels.double(), reduction='none')
    R_ = latent.size(0)
    tot = torch.zeros(R_, dtype=torch.float64, device=latent.device).index_add_(0, index.long(), loss)
    return tot / torch.bincount(index.long(), minlength=R_).clamp(min=1)


def test_step_tunes_the_latent_and_nothing_else(dev, head, inputs, replay):
    from objectcentricocccompletion_amd.occ import latent_tune
    (a0,), cache_a = _walk(head, replay, inputs, dev, 1)
    seen = {}
    hook = head.conv_fused.register_forward_hook(lambda m, i, o: seen.update(fused_in=i[0]))
    try:
        (b0,), cache_b = _walk(head, replay, inputs, dev, 1, tune_at=(0,))
    finally:
        hook.remove()
    assert set(b0) == set(a0)
    # the tuned latent is tune_latents on the untuned step's latent with tune_sample's rows and weights
    rois = _rows(inputs, [0, 3], dev)[4]
    xyz, labels, index, weights, counts = _sample(head, a0, rois, 0)
    assert counts[0] == 0 and 0 < counts[1] <= TUNE['downsample_size']       # row 0 (RoI 0) holds no point
    dec, lw = head.occ_ae_head.occ_decoder, head.occ_ae_head.loss_occ_ae.loss_weight
    assert latent_tune.supported(dec, a0['fused_roi_feats'], xyz, labels, index)
    want = latent_tune.tune_latents(dec, a0['fused_roi_feats'], xyz, labels, index, TUNE['num_iter'], weights=weights,
                                    loss_weight=lw * xyz.size(0))
    assert torch.equal(b0['fused_roi_feats'], want.to(b0['fused_roi_feats'].dtype))
    assert torch.equal(b0['fused_roi_feats'][0], a0['fused_roi_feats'][0])                 # no point: bit-unchanged
    assert float((b0['fused_roi_feats'][1] - a0['fused_roi_feats'][1]).abs().max()) > 1e-3
    # ... and nothing else: the encoder's latent and the cache are those of the run that never tuned
    assert torch.equal(b0['ori_roi_feats'], a0['ori_roi_feats']) and torch.equal(b0['nonempty_roi_mask'], a0['nonempty_roi_mask'])
    assert cache_a.pos_host == cache_b.pos_host == [1, 1] and torch.equal(cache_a.pos, cache_b.pos)
    assert all(torch.equal(x, y) for x, y in zip(cache_a.k + cache_a.v, cache_b.k + cache_b.v))
    # score and box are the head's own fuse of the tuned latent
    D = head.roi_feature_channels
    assert torch.equal(seen['fused_in'][:, :D], b0['fused_roi_feats'])
    with torch.no_grad():
        fused = head.conv_fused(torch.cat([b0['fused_roi_feats'], seen['fused_in'][:, D:]], dim=1))
        assert torch.equal(head.conv_cls(fused), b0['cls_score']) and torch.equal(head.conv_reg(fused), b0['bbox_pred'])
    assert not torch.equal(b0['cls_score'][1], a0['cls_score'][1]) and not torch.equal(b0['bbox_pred'][1], a0['bbox_pred'][1])
    assert torch.equal(b0['cls_score'][0], a0['cls_score'][0])
    # the next, untuned step of both runs: every output bit-equal
    a, _ = _walk(head, replay, inputs, dev, 2)
    b, _ = _walk(head, replay, inputs, dev, 2, tune_at=(0,))
    assert torch.equal(b[0]['fused_roi_feats'], b0['fused_roi_feats'])                     # two runs, equal bits
    for key in KEYS:
        assert torch.equal(a[1][key], b[1][key]), key


def test_observation_loss_falls_for_every_roi_with_points(dev, head, inputs, replay):
    plain, _ = _walk(head, replay, inputs, dev, 3)
    tuned, _ = _walk(head, replay, inputs, dev, 3, tune_at=(0, 1, 2))
    for t in range(3):
        rois = _rows(inputs, [t, 3 + t], dev)[4]
        xyz, labels, index, _, counts = _sample(head, plain[t], rois, t)
        before = _bce_per_roi(head, plain[t]['fused_roi_feats'], xyz, labels, index)
        after = _bce_per_roi(head, tuned[t]['fused_roi_feats'], xyz, labels, index)
        print(f'frame {t}: rows {counts}, mean BCE per RoI {[f"{v:.4f}" for v in before.tolist()]} -> '
              f'{[f"{v:.4f}" for v in after.tolist()]}')
        for r, row in enumerate((t, 3 + t)):
            if row == EMPTY:
                assert counts[r] == 0 and torch.equal(tuned[t]['fused_roi_feats'][r], plain[t]['fused_roi_feats'][r])
            else:
                assert counts[r] > 0 and float(after[r]) < float(before[r]), (t, r)


def test_forward_steps_draws_the_samples_of_the_single_steps(dev, head, inputs, replay, monkeypatch):
    ae = head.occ_ae_head
    drawn = []
    real = ae.step_sample
    monkeypatch.setattr(ae, 'step_sample', lambda *a, **k: (drawn.append(real(*a, **k)), drawn[-1])[1])
    _walk(head, replay, inputs, dev, 3, tune_at=(0, 1, 2))
    single, drawn[:] = list(drawn), []
    replay.key = 'all'
    out = head.forward_steps(*inputs[:5], [0, 0, 0, 1, 1, 1], _cache(head, dev), tune=dict(TUNE))
    torch.cuda.synchronize()
    assert len(single) == 3 and len(drawn) == 1 and out['fused_roi_feats'].shape[0] == len(PICK)
    xyz, labels, index, weights, counts = drawn[0]
    rows = 0
    for t in range(3):
        sx, sl, si, sw, sc = single[t]
        for r, row in enumerate((t, 3 + t)):                       # row of the chunked call: slot r, frame t
            assert counts[row] == sc[r]
            mine, theirs = index == row, si == r
            assert torch.equal(xyz[mine], sx[theirs]) and torch.equal(labels[mine], sl[theirs])
            assert torch.equal(weights[mine], sw[theirs])
            rows += sc[r]
    assert rows == sum(counts) > 0


def test_a_rois_gradient_does_not_depend_on_its_company(dev, head, inputs, replay):
    """The first-iteration latent gradient (debug=True, ``de``) of one RoI tuned alone and tuned as RoI 37 of 64, each
    against float64 (tests/latent_tune_ref.py) with the same weights: the two agree within twice the larger of the two
    measured errors.  In float64 the two are the same number (scale x weight = loss_weight / m_r in both calls).
    Measured on the MI355X: see DESIGN 3.19."""
    from objectcentricocccompletion_amd.occ import fused_mlp as fm, latent_tune
    plain, _ = _walk(head, replay, inputs, dev, 1)
    rois = _rows(inputs, [0, 3], dev)[4]
    xyz, labels, index, weights, counts = _sample(head, plain[0], rois, 0)
    own = index == 1                                                            # the RoI with points of that step
    x1, l1, w1 = xyz[own], labels[own], weights[own]
    m = x1.size(0)
    e1 = plain[0]['fused_roi_feats'][1:2].float()
    dec, lw = head.occ_ae_head.occ_decoder, head.occ_ae_head.loss_occ_ae.loss_weight
    K, AT = 64, 37
    g = torch.Generator().manual_seed(5)
    eK = (e1 + 0.05 * torch.randn(K, e1.size(1), generator=g).to(dev)).contiguous()
    eK[AT] = e1[0]
    xK = x1.repeat(K, 1)
    lK = torch.stack([l1 if k == AT else (torch.rand(m, generator=g) < 0.5).int().to(dev) for k in range(K)]).view(-1)
    iK = torch.arange(K, device=dev, dtype=torch.int32).repeat_interleave(m)
    wK = w1.repeat(K)
    zero = torch.zeros(m, dtype=torch.int32, device=dev)
    _, alone = latent_tune.tune_latents(dec, e1, x1, l1, zero, 1, weights=w1, loss_weight=lw * m, debug=True)
    _, company = latent_tune.tune_latents(dec, eK, xK, lK, iK, 1, weights=wK, loss_weight=lw * m * K, debug=True)
    torch.cuda.synchronize()
    layers, hd = dec._fused_layers()
    D = dec.roi_feature_channels
    P = dict(W_roi=layers[0][0].weight[:, :D], W_pe=layers[0][0].weight[:, D:], W1=layers[1][0].weight,
             W2=layers[2][0].weight, g=[ln.weight for _, ln in layers], b=[ln.bias for _, ln in layers],
             hw=hd.weight.view(-1), hb=hd.bias, eps=layers[0][1].eps, use_ln=bool(dec.use_ln),
             ln_g=dec.ln.weight if dec.use_ln else None, ln_b=dec.ln.bias if dec.use_ln else None,
             ln_eps=dec.ln.eps if dec.use_ln else 0.0)
    bound = dec.pos_encode.norm_bound if dec.pos_encode.use_norm else None
    pe = lambda x: fm.pos_encode_bf16(x, dec.pos_encode.L, bound)[:, :60]
    ref1 = R.latent_gradient(P, pe(x1), e1, zero.long(), l1, w1, lw * m, rounding='train')[0][0].detach()
    refK = R.latent_gradient(P, pe(xK), eK, iK.long(), lK, wK, lw * m * K, rounding='train')[0][AT].detach()
    norm = float(ref1.norm())
    assert float((ref1 - refK).norm()) <= 1e-9 * norm                          # float64: one number
    d1, dK = alone['de'][0].double(), company['de'][AT].double()
    err1, errK = float((d1 - ref1).norm()) / norm, float((dK - refK).norm()) / norm
    apart = float((d1 - dK).norm()) / norm
    print(f'first gradient of one RoI ({m} rows): alone {err1:.3e} and as RoI {AT} of {K} {errK:.3e} from float64, '
          f'{apart:.3e} from each other')
    assert apart <= 2 * max(err1, errK), (apart, err1, errK)


# ------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def model(dev):
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (register)
    from objectcentricocccompletion_amd.occ.occ_base import OccDecoder
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    torch.manual_seed(0)
    m = DETECTORS.build(ococcnet_model_cfg()).to(dev).eval()
    for mod in m.modules():
        if isinstance(mod, OccDecoder):
            mod.compute_dtype = torch.bfloat16
    return m


def test_step_occ_is_decoded_from_the_tuned_latent(dev, model):
    from test_gpu_online_chunk import _tracklet_inputs
    rh, bh = model.roi_head, model.roi_head.bbox_head
    kw = _tracklet_inputs(dev)
    xyz, feats, batch, frames = model._cat_points(kw['points'], kw['pts_frame_inds'])
    rois, _, cls_preds, labels_3d = rh.tracklets2rois(kw['tracklet'])
    sel = frames == 0
    call = lambda **k: rh.simple_test_step(xyz[sel], feats[sel], torch.zeros_like(batch[sel]), rois[0:1, 1:8], cls_preds[0:1],
                                           labels_3d[0:1], [0], rh.online_begin(1, dev, cap=2), **k)
    taken = []
    real = bh.forward_step
    bh.forward_step = lambda *a, **k: (taken.append((a[4], real(*a, **k))), taken[-1][1])[1]
    try:
        plain = call(occ=True)
        out = call(occ=True, tune=dict(num_iter=3, downsample_size=64))
    finally:
        del bh.forward_step
    step_rois, res = taken[-1]
    assert set(out) == set(plain) and out['fused_roi_feats'] is res['fused_roi_feats']
    occ, flags, counts = bh.get_frame_occ(out['fused_roi_feats'], step_rois, res['local_xyz'], res['roi_inds'])
    assert counts == out['occ_counts'] and torch.equal(flags, out['occ_flags']) and torch.equal(occ, out['occ'])
    scale = float(plain['fused_roi_feats'].abs().max())
    moved = float((out['fused_roi_feats'] - plain['fused_roi_feats']).abs().max())
    assert moved > 1e-3 * scale                                               # (two steps differ by 1e-6 of it untuned)
    assert float((out['ori_roi_feats'] - plain['ori_roi_feats']).abs().max()) <= 1e-4 * float(plain['ori_roi_feats'].abs().max())


def test_simple_test_under_online_step_tuning(dev, model):
    from test_gpu_online_chunk import _simple_test
    rh = model.roi_head
    seen = []
    real = rh.bbox_head._step_tuner
    rh.bbox_head._step_tuner = lambda *a, **k: (seen.append(a[0]), real(*a, **k))[1]
    rh.test_cfg['online'] = True
    try:
        plain = _simple_test(model, dev)
        assert not seen
        for chunk in (1, 4):
            rh.test_cfg['online_chunk'] = chunk
            rh.test_cfg['online_step_tuning'] = dict(num_iter=2, downsample_size=64, balance_sample=True, seed=0)
            n = len(seen)
            tuned = _simple_test(model, dev)
            assert len(seen) > n and seen[-1] == (2, 64, True, 0)
            assert set(tuned) == set(plain), chunk
    finally:
        del rh.bbox_head._step_tuner
        rh.test_cfg['online'] = False
        rh.test_cfg.pop('online_chunk', None)
        rh.test_cfg.pop('online_step_tuning', None)


def test_online_raw_step_tuning(dev, model, tmp_path):
    """tools/online_raw.py --step-tuning 2 in a child process on make_synthetic_raw's tree writes its .bin"""
    tools = os.path.join(ROOT, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import make_synthetic_raw
    root, ckpt, out = str(tmp_path / 'raw'), str(tmp_path / 'model.pth'), str(tmp_path / 'tuned.bin')
    make_synthetic_raw.main([root, '--segments', '1', '--tracklets', '2', '--frames', '4', '--background', '500'])
    torch.save(dict(state_dict=model.state_dict()), ckpt)
    p = subprocess.Popen(['timeout', '-k', '10', '300', sys.executable, 'tools/online_raw.py', CFG, ckpt,
                          os.path.join(root, 'synthetic_vehicle.yaml'), '--poses', os.path.join(root, 'poses.pkl'),
                          '--slots', '4', '--out', out, '--step-tuning', '2'], cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True)
    stdout, err = p.communicate(timeout=400)
    assert p.returncode == 0, stdout[-2000:] + err[-3000:]
    assert 'refined; wrote' in stdout and os.path.getsize(out) > 0
