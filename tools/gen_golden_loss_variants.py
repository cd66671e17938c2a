"""Generate tests/golden/ococc_loss_variants.npz: the REFERENCE's own OccBBoxHead.loss_occ
(mmdet3d/models/roi_heads/bbox_heads/ococc_bbox_head.py:608-811) with its four train_cfg switches -- contrastive_loss,
residual_loss, no_loss_for_outside, no_loss_for_observed_feats -- each alone and all four together, on the seeded scene
of oracle/synth.synth_training_scene with name-hashed weights.  The head is built as oracle/gen_golden_train.py builds it
(oracle/ref_train_shim.py and oracle/synth.py imported unchanged, eval mode), where the reference tree exists.  The
settings with residual_loss run with fused_mode='concat_residual' (upstream asserts 'residual' in it; the same parameter
shapes as the config's 'concat', so the same weights load).  Data only, no reference source.

Per setting S the file holds `S/loss_<key>` for every key of forward_train's dict (`loss_rcnn_occ_residual` also as
`S/loss_loss_rcnn_occ_residual_mean`, what mmdet's _parse_losses makes of the vector) and `S/grad_norms`: the norms of
the gradient of the sum of the means of all `loss*` entries w.r.t. the 269 parameters (`grad_names`), and
`S/counted_<key>`: how many samples the reference counted in each entry that is a mean or a ratio over samples (the
denominators of recall_* / precision_*, the samples with a weight for loss_rcnn_occ, those that are also unmatched for
loss_rcnn_occ_residual).  Once, because
they do not depend on the setting: `ori_logits` (the reference decoder's logits of ori_roi_feats at every sample) and
`face_dist` (every sample's smallest distance to a face of its RoI's box).  A sample is a BAND sample when its class or
its inside-test can turn on rounding: |ori logit| <= 4e-3 * max |ori logit| (twice the 2e-3 the project grants the
decoder's logits) or face_dist <= 1e-4 m; `band` marks them.

Asserted here, because the tests rest on it: every mask a setting exercises keeps between 5 % and 95 % of the samples,
every setting's dict differs from the default golden (tests/golden/ococc_train.npz) in the keys it is meant to affect,
and band samples are at most 2 % of all samples.

Seeds: the scene is synth_training_scene(seed=0), as for the default golden.  The weights are synth_state_dict(seed=2),
not the default golden's seed 0: whether an ori logit is above or below 0 is decided by the hashed weights of the
decoder's last layers, hardly by the scene -- with weight seeds 0, 1, 3 and 5 (and scene seeds 0-4 under weight seed 0)
every ori logit has one sign, so the observed mask keeps none or all of the samples; weight seed 2 is the first that
keeps a share inside 5-95 % (31 %) with the band under 2 % (1.35 %).  Both seeds are recorded in the file (`seed`,
`weight_seed`) and the tests load the weights of that seed.  "Differs from the default" is checked against a run of the
same head with no switch on, which for the seeds (0, 0) is asserted to be the committed default golden.

usage: python tools/gen_golden_loss_variants.py [--seed N] [--weight-seed N]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_train_shim as T  # noqa: E402
from oracle import synth  # noqa: E402
from oracle.gen_golden_train import to_ref_tracklets  # noqa: E402

SWITCHES = ('contrastive_loss', 'residual_loss', 'no_loss_for_outside', 'no_loss_for_observed_feats')
SETTINGS = {'contrastive': ('contrastive_loss',), 'residual': ('residual_loss',), 'outside': ('no_loss_for_outside',),
            'observed': ('no_loss_for_observed_feats',), 'all': SWITCHES}
OCC_KEYS = ('loss_rcnn_occ', 'recall_neg', 'recall_pos', 'precision_neg', 'precision_pos')
AFFECTS = {'contrastive': (), 'residual': OCC_KEYS[:1], 'outside': OCC_KEYS, 'observed': OCC_KEYS, 'all': OCC_KEYS}
NEW_KEYS = {'contrastive': ('loss_contrastive_feats',), 'residual': ('num_unmatched', 'loss_rcnn_occ_residual'),
            'outside': (), 'observed': (), 'all': ('loss_contrastive_feats', 'num_unmatched', 'loss_rcnn_occ_residual')}
LOGIT_BAND, FACE_BAND, MAX_BAND_SHARE = 4e-3, 1e-4, 0.02


class Spy(object):
    """records what loss_occ hands its decoder and its loss module (instance attributes in front of the methods)"""

    def __init__(self, bbox_head):
        self.head, self.dec, self.crit = bbox_head, bbox_head.occ_ae_head.occ_decoder, bbox_head.loss_occ_comp
        self.decodes, self.crits, self.args, self.on = [], [], None, True
        dec_fwd, crit_fwd, loss_occ = self.dec.occ_forward, self.crit.forward, bbox_head.loss_occ

        def occ_forward(feats, xyz):
            out = dec_fwd(feats, xyz)
            if self.on:
                self.decodes.append((torch.is_grad_enabled(), feats.dim(), xyz.detach().clone(), out.detach().clone()))
            return out

        def crit_forward(pred, label, weight=None, **kw):
            self.crits.append((label.detach().clone(), weight.detach().clone()))
            return crit_fwd(pred, label, weight, **kw)

        def spy_loss_occ(rois, roi_features, ori_roi_feats, pos_batch_idx, pos_gt_bboxes, reg_mask, nonempty, *a, **kw):
            self.args = (rois.detach().clone(), ori_roi_feats.detach().clone(), (reg_mask > 0) & nonempty)
            return loss_occ(rois, roi_features, ori_roi_feats, pos_batch_idx, pos_gt_bboxes, reg_mask, nonempty, *a, **kw)

        self.dec.occ_forward, self.crit.forward, bbox_head.loss_occ = occ_forward, crit_forward, spy_loss_occ

    def clear(self):
        self.decodes, self.crits, self.args = [], [], None


def run_setting(head, c, samples, spy, name):
    on = SETTINGS[name]
    bh = head.bbox_head
    for k in SWITCHES:
        bh.train_cfg[k] = k in on
    bh.fused_mode = 'concat_residual' if 'residual_loss' in on else 'concat'
    spy.clear()
    trks, cands, occs, occ_scores = to_ref_tracklets(c, samples)
    pts = [torch.from_numpy(s['points']) for s in samples]
    cat = torch.cat(pts, 0)
    batch_idx = torch.cat([torch.full((len(p),), i, dtype=torch.long) for i, p in enumerate(pts)])
    frame_inds = torch.cat([torch.from_numpy(s['pts_frame_inds']) for s in samples])
    torch.manual_seed(123)
    head.zero_grad()
    losses = head.forward_train(cat[:, :3], cat[:, 3:], batch_idx, frame_inds.clone(), None, trks, cands, occs, occ_scores)
    out = {}
    for k, v in losses.items():
        out[f'{name}/loss_{k}'] = v.detach().numpy().astype(np.float32)
    if 'loss_rcnn_occ_residual' in losses:
        out[f'{name}/loss_loss_rcnn_occ_residual_mean'] = losses['loss_rcnn_occ_residual'].mean().detach().numpy().astype(np.float32)
    total = sum(v.mean() for k, v in losses.items() if 'loss' in k)   # tools/train.py:136, mmdet's _parse_losses
    total.backward()
    names, norms = [], []
    for n, p in bh.named_parameters():
        names.append(n)
        norms.append(0.0 if p.grad is None else float(p.grad.double().norm()))
    out[f'{name}/grad_norms'] = np.asarray(norms, np.float64)
    # the samples: the main decode is the one under autograd on [M, K, D] features
    main = [d for d in spy.decodes if d[0] and d[1] == 3]
    assert len(main) == 1 + ('residual_loss' in on), len(main)
    xyz = main[-1][2]
    rois, ori, pos = spy.args
    M, K, _ = xyz.shape
    size = rois[pos][:, 4:7]
    assert size.shape == (M, 3)
    spy.on = False
    with torch.no_grad():
        ori_logits = spy.dec.occ_forward(ori[pos][:, None, :].repeat(1, K, 1), xyz).reshape(-1)
    spy.on = True
    for d in spy.decodes:   # the reference's own ori decodes (under no_grad) are what was just recomputed
        if not d[0]:
            assert torch.equal(d[3].reshape(-1), ori_logits)
    face = ((xyz.abs() - size[:, None, :] / 2).abs()).min(-1).values.reshape(-1)
    inside = ((xyz >= -size[:, None, :] / 2).all(-1) & (xyz <= size[:, None, :] / 2).all(-1)).reshape(-1)
    labels, weights = spy.crits[-1]
    # how many samples each entry that is a mean over samples counts (what one flipped band sample weighs in it)
    labels, weights = labels.reshape(-1), weights.reshape(-1)
    valid, pred = weights > 0, (main[0][3].reshape(-1).sigmoid() > spy.dec.pos_thresh)
    unmatched = labels != (ori_logits.sigmoid() > spy.dec.pos_thresh).long()
    counted = dict(recall_neg=valid & (labels == 0), recall_pos=valid & (labels == 1), precision_neg=valid & ~pred,
                   precision_pos=valid & pred, loss_rcnn_occ=valid, loss_rcnn_occ_residual=valid & unmatched)
    for k, m in counted.items():
        out[f'{name}/counted_{k}'] = np.asarray(int(m.sum()), np.int64)
    info = dict(names=names, xyz=xyz, ori_logits=ori_logits, face=face, inside=inside, labels=labels.reshape(-1),
                weights=weights.reshape(-1), losses=losses)
    return out, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=0, help='of synth_training_scene')
    ap.add_argument('--weight-seed', type=int, default=2, help='of synth_state_dict (the name-hashed weights)')
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    head, c = T.build_reference_roi_head()
    if args.weight_seed:
        shapes = {k: tuple(v.shape) for k, v in head.bbox_head.state_dict().items()}
        head.bbox_head.load_state_dict(synth.synth_state_dict(shapes, seed=args.weight_seed))
    head.eval()
    samples = synth.synth_training_scene(seed=args.seed)
    spy = Spy(head.bbox_head)
    SETTINGS['default'] = ()   # (run for the comparison below; not written)
    plain, _ = run_setting(head, c, samples, spy, 'default')
    del SETTINGS['default']
    default = {k[len('default/'):]: v for k, v in plain.items() if '/loss_' in k}
    if args.seed == 0 and args.weight_seed == 0:   # the committed default golden is this run
        committed = np.load(os.path.join(ROOT, 'tests', 'golden', 'ococc_train.npz'))
        assert sorted(default) == sorted(k for k in committed.files if k.startswith('loss_'))
        assert all(np.array_equal(default[k], committed[k]) for k in default)
    out, infos = {'seed': np.asarray(args.seed), 'weight_seed': np.asarray(args.weight_seed),
                  'settings': np.array(list(SETTINGS))}, {}
    for name in SETTINGS:
        o, infos[name] = run_setting(head, c, samples, spy, name)
        out.update(o)
        print(name, {k: np.round(v.reshape(-1)[:3], 5).tolist() for k, v in o.items() if 'grad' not in k})
    ref = infos['contrastive']   # no mask on: the plain weights
    for name, i in infos.items():
        assert torch.equal(i['xyz'], ref['xyz']) and torch.equal(i['ori_logits'], ref['ori_logits'])
        assert torch.equal(i['labels'], ref['labels']) and i['names'] == ref['names']
    n = ref['labels'].numel()
    ori, face, inside, labels, base = ref['ori_logits'], ref['face'], ref['inside'], ref['labels'], ref['weights']
    unobserved = ~(ori.sigmoid() > head.bbox_head.occ_ae_head.occ_decoder.pos_thresh)
    unmatched = labels != (~unobserved).long()
    share = lambda m: float(m.float().mean())
    print(f'ori logits min {float(ori.min()):.4f} median {float(ori.median()):.4f} max {float(ori.max()):.4f}')
    print(f'{n} samples: base weight {share(base > 0):.3f}, inside {share(inside):.3f}, unobserved {share(unobserved):.3f}, '
          f'unmatched {share(unmatched):.3f}')
    for what, m in (('inside', inside), ('unobserved', unobserved), ('unmatched', unmatched)):
        assert 0.05 <= share(m) <= 0.95, (what, share(m))
    # the weights the reference used are the masks restated here
    assert torch.equal(infos['outside']['weights'], base * inside.float())
    assert torch.equal(infos['observed']['weights'], base * unobserved.float())
    assert torch.equal(infos['all']['weights'], base * inside.float() * unobserved.float())
    assert torch.equal(infos['residual']['weights'], base)
    for name in ('residual', 'all'):
        assert float(out[f'{name}/loss_num_unmatched']) == float(unmatched.sum())
        assert out[f'{name}/loss_loss_rcnn_occ_residual'].size == int(unmatched.sum())
    band = (ori.abs() <= LOGIT_BAND * float(ori.abs().max())) | (face <= FACE_BAND)
    print(f'band samples: {int(band.sum())} of {n} ({share(band):.4f}); max |ori logit| {float(ori.abs().max()):.4f}')
    assert share(band) <= MAX_BAND_SHARE, share(band)
    for name in SETTINGS:
        keys = {k[len(name) + 6:] for k in out if k.startswith(name + '/loss_')} - {'loss_rcnn_occ_residual_mean'}
        old = {k[5:] for k in default}
        assert keys == old | set(NEW_KEYS[name]), (name, keys ^ old)
        for k in old:
            a, b = out[f'{name}/loss_{k}'], default['loss_' + k]
            same = a.shape == b.shape and np.array_equal(a, b)
            if k in AFFECTS[name]:
                assert not same, (name, k, 'is the default')
            elif name != 'residual' and name != 'all':     # (another fused_mode: every head output moves)
                assert same, (name, k, 'moved')
    out['grad_names'] = np.array(ref['names'])
    out['ori_logits'], out['face_dist'], out['band'] = ori.numpy(), face.numpy(), band.numpy()
    dst = os.path.join(ROOT, 'tests', 'golden', 'ococc_loss_variants.npz')
    np.savez_compressed(dst, **out)
    print('wrote', dst, os.path.getsize(dst), 'bytes')


if __name__ == '__main__':
    main()
