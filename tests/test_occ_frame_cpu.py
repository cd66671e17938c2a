"""Completed occupancy of an online step without a GPU: the operator chain occ_ops.occ_frame_select_aten on CPU tensors
against the plain restatement of tests/occ_frame_ref.py (the input tests/test_gpu_occ_frame.py runs the kernels on), its
observed cells against OccAutoEncoder.sample_observation, the argument checks of both operators, what the step methods
report on the host, and the declarations of the three exports."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import occ_frame_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ('ococc_occ_frame_mark', 'ococc_occ_frame_count', 'ococc_occ_frame_fill')


@pytest.fixture(scope='module', autouse=True)
def _generators_as_found():
    """later tests of the suite initialise networks from torch's global generators without seeding them"""
    cpu = torch.get_rng_state()
    yield
    torch.set_rng_state(cpu)


def _aten(case, **kw):
    from objectcentricocccompletion_amd.occ import occ_ops
    sizes, dims, start, total = occ_ops.dense_grid_layout(case.wlh, ref.V, case.scale, case.offset)
    assert (dims.long().prod(1)).tolist() == ref.CELLS and total == case.total        # the cases are what they claim
    return occ_ops.occ_frame_select_aten(case.logits, sizes, dims, start, total, ref.V, case.pos_thresh, case.rois,
                                         case.local_xyz, case.pts_roi, case.scale, case.offset, **kw)


def _check(got, exp, bitwise_xyz=True):
    out, flags, counts = got
    assert counts == exp.counts
    assert out.dtype == torch.float32 and flags.dtype == torch.uint8 and tuple(out.shape) == (sum(counts), 4)
    assert np.array_equal(flags.numpy(), exp.flags)
    assert np.array_equal(out[:, 3].numpy(), exp.out[:, 3])
    if bitwise_xyz:
        assert out[:, :3].numpy().tobytes() == exp.out[:, :3].tobytes()


@pytest.mark.parametrize('pos_thresh', [0.5, 0.3])
@pytest.mark.parametrize('enlarge', ref.ENLARGE)
def test_aten_chain_equals_the_restatement(enlarge, pos_thresh):
    case = ref.make_case(enlarge, pos_thresh)
    assert 180 <= case.local_xyz.size(0) <= 220
    prob, cos, sin = case.logits.sigmoid(), torch.cos(case.rois[:, 7]), torch.sin(case.rois[:, 7])
    exp = ref.run_ref(case, prob, cos, sin, row_keep=case.row_keep)
    _check(_aten(case, row_keep=case.row_keep), exp)
    c = exp.counts
    assert c[ref.FILTERED] == 0 and c[ref.UNSEEN] == 0 and c[ref.ALL_POSITIVE] == 1024 and 0 < c[ref.SEEN_ONLY] <= 8
    first = exp.flags[:c[ref.SEEN_ONLY]]
    assert (first == 2).all() and set(np.unique(exp.flags)) == {1, 2, 3}
    _check(_aten(case), ref.run_ref(case, prob, cos, sin))                              # nothing filtered
    assert ref.run_ref(case, prob, cos, sin).counts[ref.FILTERED] == 60
    off = ref.run_ref(case, prob, cos, sin, row_keep=case.row_keep, observed=False)
    _check(_aten(case, row_keep=case.row_keep, observed=False), off)
    assert off.counts[ref.SEEN_ONLY] == 0 and not (off.flags & 2).any()
    # the observed cells are the cells sample_observation labels 1
    from objectcentricocccompletion_amd.heads import OccAutoEncoder
    ae = types.SimpleNamespace(compensate_encoder_coors=True, voxel_size=ref.V, scale_wlh=case.scale, offset_wlh=case.offset)
    _, labels, _ = OccAutoEncoder.sample_observation(ae, case.local_xyz, case.rois, case.pts_roi, downsample_size=-1,
                                                     balance_sample=False)
    assert np.array_equal(labels.numpy(), exp.seen.astype(np.int64)) and 150 < int(labels.sum()) < case.local_xyz.size(0)
    full = ref.run_ref(case, prob, cos, sin)
    assert np.array_equal(np.sort(full.cell[(full.flags & 2) != 0]), np.flatnonzero(exp.seen))
    # no point at all
    none = types.SimpleNamespace(**dict(vars(case), local_xyz=case.local_xyz[:0], pts_roi=case.pts_roi[:0]))
    _check(_aten(none, row_keep=case.row_keep), ref.run_ref(case, prob, cos, sin, row_keep=case.row_keep, points=False))


def test_aten_chain_with_a_matrix_stays_within_the_derived_bound():
    """identity and a yawed pose 150 m from the origin; the chain multiplies with torch.bmm, whose summation order is its
    own: held to 3u / (1 - 3u) * (|t0 x| + |t1 y| + |t2 z| + |t3|) against float64 of the same f32 matrix"""
    case = ref.make_case(ref.ENLARGE[0], 0.5)
    plain = _aten(case, row_keep=case.row_keep)
    xyz = plain[0][:, :3].numpy()
    rows = np.repeat(np.arange(case.R), plain[2])
    for pose in (ref.yawed_pose(0.0, 0.0, 0.0, 0.0), ref.yawed_pose(0.7, 120.0, -90.0, 1.5)):
        T = torch.from_numpy(np.tile(pose, (case.R, 1)))
        T[1] = torch.from_numpy(ref.yawed_pose(-2.1, -100.0, 111.8, -0.5)) if pose[3] else T[1]   # (a matrix per row)
        got = _aten(case, row_keep=case.row_keep, transforms=T)
        assert got[2] == plain[2] and torch.equal(got[1], plain[1]) and torch.equal(got[0][:, 3], plain[0][:, 3])
        t = T.numpy()[rows]
        err = np.abs(got[0][:, :3].numpy().astype(np.float64) - ref.apply64(t, xyz))
        bound = ref.matrix_bound(t, xyz)
        print(f'pose at {np.hypot(pose[3], pose[7]):.0f} m: largest error {err.max():.3e}, '
              f'largest error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}')
        assert (err <= bound).all()
        _check(got, ref.run_ref(case, case.logits.sigmoid(), torch.cos(case.rois[:, 7]), torch.sin(case.rois[:, 7]),
                                row_keep=case.row_keep, transforms=T), bitwise_xyz=False)


def test_two_logit_decoders_take_the_chain():
    case = ref.make_case(ref.ENLARGE[0], 0.5)
    lg = case.logits.clone()
    lg[case.near] = 1.0          # (l1 > l0 and sigmoid(l1 - l0) > 0.5 part ways within a denormal of zero)
    case = types.SimpleNamespace(**dict(vars(case), logits=lg))
    two = types.SimpleNamespace(**dict(vars(case), logits=torch.stack([torch.zeros_like(lg), lg], 1)))
    a, b = _aten(two, row_keep=case.row_keep), _aten(case, row_keep=case.row_keep)
    assert a[2] == b[2] and torch.equal(a[1], b[1]) and torch.equal(a[0][:, :3], b[0][:, :3])
    assert torch.allclose(a[0][:, 3], b[0][:, 3], atol=1e-6)


def test_wrong_dtypes_and_shapes_raise():
    from objectcentricocccompletion_amd._lib import OcoccError
    from objectcentricocccompletion_amd.occ import occ_ops
    case = ref.make_case(ref.ENLARGE[0], 0.5)
    sizes, dims, start, total = occ_ops.dense_grid_layout(case.wlh, ref.V, case.scale, case.offset)
    good = dict(logits=case.logits, sizes=sizes, dims=dims, start=start, total=total, voxel_size=ref.V, pos_thresh=0.5,
                rois=case.rois, local_xyz=case.local_xyz, pts_roi=case.pts_roi, row_keep=case.row_keep,
                transforms=torch.zeros(case.R, 12))
    bad = [dict(logits=case.logits.double()), dict(logits=case.logits[:-1]), dict(logits=case.logits.view(-1, 1, 1)),
           dict(dims=dims.long()), dict(start=start[:-1]), dict(sizes=sizes.double()), dict(rois=case.rois[:, :7]),
           dict(rois=case.rois[:-1]), dict(rois=None), dict(local_xyz=case.local_xyz.double()),
           dict(local_xyz=case.local_xyz[:, :2]), dict(pts_roi=case.pts_roi.float()), dict(pts_roi=case.pts_roi[:-1]),
           dict(row_keep=case.row_keep.float()), dict(row_keep=case.row_keep[:-1]), dict(transforms=torch.zeros(case.R, 9)),
           dict(transforms=torch.zeros(case.R, 12, dtype=torch.float64))]
    for fn in (occ_ops.occ_frame_select, occ_ops.occ_frame_select_aten):
        for change in bad:
            with pytest.raises(OcoccError, match=fn.__name__):
                fn(**dict(good, **change))
    with pytest.raises(OcoccError, match='2'):                                       # the kernels take one logit
        occ_ops.occ_frame_select(**dict(good, logits=torch.zeros(total, 2)))
    with pytest.raises(OcoccError, match='no CPU fallback'):                         # ... and no CPU tensors
        occ_ops.occ_frame_select(**good)
    out, flags, counts = occ_ops.occ_frame_select_aten(**dict(good, transforms=None))
    assert sum(counts) == out.size(0) == flags.size(0) > 1024
    # no RoI at all
    e = occ_ops.dense_grid_layout(case.wlh[:0], ref.V)
    out, flags, counts = occ_ops.occ_frame_select_aten(torch.zeros(0), e[0], e[1], e[2], 0, ref.V, 0.5, case.rois[:0],
                                                       case.local_xyz[:0], case.pts_roi[:0])
    assert tuple(out.shape) == (0, 4) and tuple(flags.shape) == (0,) and counts == []


def test_decoder_refuses_cpu_tensors():
    """OccDecoder.get_frame_occ decodes on the device only: CPU tensors are refused before anything runs; no RoI is an
    empty result"""
    from objectcentricocccompletion_amd._lib import OcoccError
    from objectcentricocccompletion_amd.occ.occ_base import OccDecoder
    dec = OccDecoder(32, [16, 16], pos_encode_L=4, norm_cfg=dict(type='LN', eps=1e-3), act='gelu', occ_dropout=0.0,
                     use_ln=True).eval()
    rois = torch.tensor([[0, 1.0, 2.0, 0.5, 1.1, 0.9, 0.7, 0.3], [0, -3.0, 1.0, 0.0, 0.5, 0.7, 0.9, -1.0]])
    xyz, inds = torch.zeros(3, 3), torch.tensor([0, 1, 1], dtype=torch.int32)
    with pytest.raises(OcoccError, match='no CPU fallback'):
        dec.get_frame_occ(torch.zeros(2, 32), rois, 0.2, [1.0] * 3, [0.0] * 3, xyz, inds)
    out, flags, counts = dec.get_frame_occ(torch.zeros(0, 32), rois[:0], 0.2, [1.0] * 3, [0.0] * 3, xyz[:0], inds[:0])
    assert tuple(out.shape) == (0, 4) and flags.dtype == torch.uint8 and counts == []


@pytest.fixture(scope='module')
def model():
    from objectcentricocccompletion_amd import heads, point_pool, roi_head  # noqa: F401 (register)
    from objectcentricocccompletion_amd.ococcnet_cfg import ococcnet_model_cfg
    from objectcentricocccompletion_amd.registry import DETECTORS
    return DETECTORS.build(ococcnet_model_cfg()).eval()


def _frame(n=1):
    return dict(pts_xyz=torch.zeros(4, 3), pts_feats=torch.zeros(4, 7), pts_batch_idx=torch.zeros(4, dtype=torch.long),
                boxes=torch.ones(n, 7), scores=torch.ones(n), labels=torch.zeros(n, dtype=torch.long))


def test_steps_with_occ_report_on_the_host_as_the_plain_calls_do(model):
    from objectcentricocccompletion_amd import _lib as L
    rh = model.roi_head
    state = rh.online_begin(3, 'cpu', cap=2)
    for kw in (dict(), dict(occ=True)):
        with pytest.raises(L.OcoccError, match='duplicate'):
            rh.simple_test_step(**_frame(2), slot=[1, 1], state=state, **kw)
        with pytest.raises(L.OcoccError, match='CPU tensor'):
            rh.simple_test_step(**_frame(2), slot=[0, 2], state=state, **kw)
        f = _frame(2)
        f['pts_row_idx'] = f.pop('pts_batch_idx')
        with pytest.raises(L.OcoccError, match='CPU tensor'):
            rh.simple_test_steps(**f, slot_rows=[0, 0], state=state, **kw)
        with pytest.raises(L.OcoccError, match='CPU tensor'):
            rh.simple_test_scene_step(torch.zeros(4, 6), np.eye(4), torch.ones(2, 7), torch.ones(2),
                                      torch.zeros(2, dtype=torch.long), [0, 2], state, **kw)
        state.reset()
    assert state.frames == [0, 0, 0]
    assert rh.online_occ_cfg() == dict(observed=True, chunk=1 << 20)
    for wrong in (dict(observed=True, rows=3), dict(chunk=0), dict(chunk=True), [1]):
        rh.test_cfg['online_occ'] = wrong
        try:
            with pytest.raises(ValueError, match='online_occ'):
                rh.online_occ_cfg()
        finally:
            del rh.test_cfg['online_occ']


def test_without_occ_the_result_has_the_keys_it_had(model, monkeypatch):
    """the step methods behind stubbed head calls: without ``occ`` the head is called as before (no new keyword reaches
    it), nothing of the occupancy path is touched, and the result has exactly the six keys; with it, three more"""
    from objectcentricocccompletion_amd import _lib as L
    rh, head = model.roi_head, model.roi_head.bbox_head
    n = 2
    res = dict(cls_score=torch.zeros(n, 1), bbox_pred=torch.zeros(n, 7), nonempty_roi_mask=torch.ones(n, dtype=torch.bool),
               fused_roi_feats=torch.zeros(n, 4), ori_roi_feats=torch.zeros(n, 4))
    seen = []

    def forward_step(*a, **k):
        seen.append(dict(k))
        return dict(res, **(dict(local_xyz=torch.zeros(1, 3), roi_inds=torch.zeros(1, dtype=torch.int32))
                            if k.get('return_points') else {}))

    def no_occ(*a, **k):
        raise AssertionError('the occupancy path was entered')
    monkeypatch.setattr(L, 'require_device', lambda *t: None)
    monkeypatch.setattr(rh, '_pool_points', lambda *a: (None, None, None, None))
    monkeypatch.setattr(head, 'forward_step', forward_step)
    monkeypatch.setattr(head, 'forward_steps', lambda *a, **k: forward_step(*a, **k))
    monkeypatch.setattr(head, 'get_bboxes_from_tracklet', lambda *a, **k: [(torch.zeros(n, 7), torch.zeros(n), torch.zeros(n),
                                                                          torch.ones(n, dtype=torch.bool))])
    monkeypatch.setattr(head, 'get_frame_occ', no_occ)
    state = rh.online_begin(3, 'cpu', cap=4)
    keys = {'boxes', 'scores', 'labels', 'valid', 'fused_roi_feats', 'ori_roi_feats'}
    assert set(rh.simple_test_step(**_frame(n), slot=[0, 2], state=state)) == keys
    f = _frame(n)
    f['pts_row_idx'] = f.pop('pts_batch_idx')
    assert set(rh.simple_test_steps(**f, slot_rows=[1, 1], state=state)) == keys
    assert seen == [{}, {}]
    calls = []

    def frame_occ(feats, rois, xyz, inds, **k):
        calls.append(k)
        return torch.zeros(3, 4), torch.ones(3, dtype=torch.uint8), [1, 2]
    monkeypatch.setattr(head, 'get_frame_occ', frame_occ)
    out = rh.simple_test_step(**_frame(n), slot=[0, 2], state=state, occ=True)
    assert set(out) == keys | {'occ', 'occ_flags', 'occ_counts'} and out['occ_counts'] == [1, 2]
    assert seen[-1] == dict(return_points=True)
    assert calls[-1]['row_keep'] is None and calls[-1]['transforms'] is None and calls[-1]['observed'] is True
    rh.test_cfg['filter_empty_roi'] = True
    rh.test_cfg['online_occ'] = dict(observed=False, chunk=4096)
    try:
        out = rh.simple_test_steps(**f, slot_rows=[1, 1], state=state, occ=True)
    finally:
        del rh.test_cfg['filter_empty_roi'], rh.test_cfg['online_occ']
    assert set(out) == keys | {'occ', 'occ_flags', 'occ_counts'}
    assert calls[-1]['row_keep'] is res['nonempty_roi_mask'] and calls[-1]['observed'] is False and calls[-1]['chunk'] == 4096


def test_exports_declared_bound_and_documented():
    from objectcentricocccompletion_amd import _lib
    with open(os.path.join(ROOT, 'include', 'ococc_hip.h')) as f:
        header = f.read()
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
        integration = f.read()
    for name in EXPORTS:
        m = re.search(r'\bint %s\(([^;]*)\);' % name, header)
        assert m, f'{name} is not declared in include/ococc_hip.h'
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert callable(getattr(_lib.lib, name))
        assert any(f'`{name}`' in line and line.startswith('|') for line in integration.splitlines()), name
    assert 'occ_ae_head.py:65-126' in header and 'occ_base.py:238-342' in header          # the reference lines replaced
    assert 'occ_frame.hip' in open(os.path.join(ROOT, 'objectcentricocccompletion_amd', 'csrc', 'Makefile')).read()
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'OCOCC_OCC_FRAME_KERNEL' in readme and '--save-occ' in readme
    assert '3.18' in open(os.path.join(ROOT, 'DESIGN.md')).read()


def test_exports_check_their_arguments_before_any_launch():
    from objectcentricocccompletion_amd import _lib as L
    lib = L.lib
    assert lib.ococc_occ_frame_mark(None, None, 0, None, None, None, 0, 0.2, None, 0, None) == 0
    assert lib.ococc_occ_frame_mark(None, None, -1, None, None, None, 0, 0.2, None, 0, None) == -1
    assert lib.ococc_occ_frame_mark(None, None, 5, None, None, None, 2, 0.0, None, 10, None) == -1
    assert b'voxel_size' in lib.ococc_last_error()
    assert lib.ococc_occ_frame_mark(None, None, 5, None, None, None, 2, 0.2, None, 10, None) == -1
    assert b'observed' in lib.ococc_last_error()
    assert lib.ococc_occ_frame_count(None, None, None, 0, None, 0, 0.5, None, None, 0, None, None) == 0
    assert lib.ococc_occ_frame_count(None, None, None, 5000, None, 3, 0.5, None, None, 6, None, None) == -1
    assert b'max_tiles' in lib.ococc_last_error()
    assert lib.ococc_occ_frame_count(None, None, None, 5000, None, 3, 0.5, None, None, 7, None, None) == -1
    assert b'null pointer' in lib.ococc_last_error()
    fill = lambda R, stride, n_out=0: lib.ococc_occ_frame_fill(None, None, None, 10, None, None, R, 0.5, None, R + 1, None,
                                                               None, 0.2, None, stride, None, None, None, None, None, n_out,
                                                               None)
    assert fill(0, 0) == 0 and fill(2, 8) == 0                                          # no RoI; no row to write
    assert fill(2, 6) == -1 and b'roi_stride' in lib.ococc_last_error()
    assert fill(2, 8, n_out=4) == -1 and b'null pointer' in lib.ococc_last_error()
    assert fill(2, 8, n_out=-1) == -1


def test_tool_lists_the_flag():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'online_raw.py'), '--help'], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and '--save-occ DIR' in out.stdout
