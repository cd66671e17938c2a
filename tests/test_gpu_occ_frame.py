"""GPU suite: csrc/occ_frame.hip (ococc_occ_frame_mark / _count / _fill behind occ_ops.occ_frame_select) against the plain
restatement of tests/occ_frame_ref.py, on synthetic logits and no model.  Six RoIs whose grids give every tile shape (12
cells, exactly 1024, 1040, 2057, a filtered RoI, an RoI with no selected cell), about 200 points with the edge cases of
the rasterisation, voxel 0.2.  Counts, flags, order, the probability column and the xyz without a matrix are exact; the
matrix step is held to the derived bound of three products and three sums.  The restatement takes cos, sin and the
sigmoid from torch on the same device (tests/test_gpu_occ_export.py pins the kernels' sigmoid to ATen's)."""
import types

import numpy as np
import pytest
import torch

import occ_frame_ref as ref

pytestmark = pytest.mark.gpu


def _on(case, dev):
    t = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in vars(case).items()}
    return types.SimpleNamespace(**t)


def _layout(c):
    from objectcentricocccompletion_amd.occ import occ_ops
    sizes, dims, start, total = occ_ops.dense_grid_layout(c.wlh, ref.V, c.scale, c.offset)
    assert dims.long().prod(1).tolist() == ref.CELLS and total == c.total                # the cases are what they claim
    return sizes, dims, start, total


def _run(fn, c, points=True, **kw):
    n = c.local_xyz.size(0) if points else 0
    return fn(c.logits, *_layout(c), ref.V, c.pos_thresh, c.rois, c.local_xyz[:n], c.pts_roi[:n], c.scale, c.offset, **kw)


def _assert_equal(got, exp, xyz=True):
    out, flags, counts = got
    assert counts == exp.counts
    assert out.dtype == torch.float32 and flags.dtype == torch.uint8 and tuple(out.shape) == (sum(counts), 4)
    assert tuple(flags.shape) == (sum(counts),)
    assert np.array_equal(flags.cpu().numpy(), exp.flags)
    o = out.cpu().numpy()
    assert o[:, 3].tobytes() == exp.out[:, 3].tobytes()                                    # the probability column
    if xyz:
        assert o[:, :3].tobytes() == exp.out[:, :3].tobytes()                              # bit for bit, hence the order


@pytest.fixture(scope='module', params=[(e, p) for e in ref.ENLARGE for p in (0.5, 0.3)],
                ids=lambda v: f'scale{v[0][0][0]}-thresh{v[1]}')
def case(request, dev):
    """the input, the device's cos / sin / sigmoid, and the restatement -- computed once per parameter"""
    c = _on(ref.make_case(*request.param), dev)
    c.host = ref.make_case(*request.param)
    c.prob, c.cos, c.sin = c.logits.sigmoid(), torch.cos(c.rois[:, 7]), torch.sin(c.rois[:, 7])
    c.exp = ref.run_ref(c.host, c.prob, c.cos, c.sin, row_keep=c.host.row_keep)
    return c


def test_kernels_equal_the_restatement(case):
    from objectcentricocccompletion_amd.occ import occ_ops
    c = case
    assert 180 <= c.local_xyz.size(0) <= 220
    got = _run(occ_ops.occ_frame_select, c, row_keep=c.row_keep)
    _assert_equal(got, c.exp)
    n = c.exp.counts
    assert n[ref.FILTERED] == 0 and n[ref.UNSEEN] == 0 and n[ref.ALL_POSITIVE] == 1024 and 0 < n[ref.SEEN_ONLY] <= 8
    assert (c.exp.flags[:n[ref.SEEN_ONLY]] == 2).all() and set(np.unique(c.exp.flags)) == {1, 2, 3}
    # (the logits at the threshold and its two neighbours, c.near, are decided as the restatement decides them)
    assert c.near.numel() >= 50
    # two runs: equal bytes
    again = _run(occ_ops.occ_frame_select, c, row_keep=c.row_keep)
    assert got[0].cpu().numpy().tobytes() == again[0].cpu().numpy().tobytes()
    assert got[1].cpu().numpy().tobytes() == again[1].cpu().numpy().tobytes() and got[2] == again[2]
    # bool row_keep, int64 RoI indices, [N, 1] logits: the same call
    alt = types.SimpleNamespace(**dict(vars(c), logits=c.logits.view(-1, 1), pts_roi=c.pts_roi.long()))
    _assert_equal(_run(occ_ops.occ_frame_select, alt, row_keep=c.row_keep.bool()), c.exp)
    # nothing filtered: the filtered RoI's 60 positive cells appear
    full = ref.run_ref(c.host, c.prob, c.cos, c.sin)
    _assert_equal(_run(occ_ops.occ_frame_select, c), full)
    assert full.counts[ref.FILTERED] == 60
    # M = 0
    _assert_equal(_run(occ_ops.occ_frame_select, c, points=False, row_keep=c.row_keep),
                  ref.run_ref(c.host, c.prob, c.cos, c.sin, row_keep=c.host.row_keep, points=False))


def test_observed_off_equals_occ_select(case):
    """without the observation the rows are those of the export's selection, bit for bit (xyz and probability)"""
    from objectcentricocccompletion_amd.occ import occ_ops
    c = case
    out, flags, counts = _run(occ_ops.occ_frame_select, c, observed=False)
    _assert_equal((out, flags, counts), ref.run_ref(c.host, c.prob, c.cos, c.sin, observed=False))
    exp, exp_counts = occ_ops.occ_select(c.logits, *_layout(c), ref.V, c.pos_thresh, c.rois, with_score=True)
    assert counts == exp_counts and bool((flags == 1).all())
    assert out.cpu().numpy().tobytes() == exp.cpu().numpy().tobytes()


def test_matrix_step(case):
    """identity: bit for bit again; a yawed pose 150 m from the origin (and another one for one RoI): within
    3u / (1 - 3u) * (|t0 x| + |t1 y| + |t2 z| + |t3|) per coordinate of float64 of the same f32 matrix -- and equal to
    the restatement, which rounds where the kernel rounds"""
    from objectcentricocccompletion_amd.occ import occ_ops
    c = case
    plain = c.exp.out[:, :3]
    rows = np.repeat(np.arange(c.R), c.exp.counts)
    eye = torch.from_numpy(np.tile(ref.yawed_pose(0.0, 0.0, 0.0, 0.0), (c.R, 1)))
    got = _run(occ_ops.occ_frame_select, c, row_keep=c.row_keep, transforms=eye.to(c.logits.device))
    _assert_equal(got, c.exp)
    far = torch.from_numpy(np.tile(ref.yawed_pose(0.7, 120.0, -90.0, 1.5), (c.R, 1)))
    far[1] = torch.from_numpy(ref.yawed_pose(-2.1, -100.0, 111.8, -0.5))
    assert abs(float(np.hypot(120.0, 90.0)) - 150.0) < 1e-9
    for T in (far, far.view(c.R, 3, 4)):
        got = _run(occ_ops.occ_frame_select, c, row_keep=c.row_keep, transforms=T.to(c.logits.device))
        t = far.numpy()[rows]
        err = np.abs(got[0][:, :3].cpu().numpy().astype(np.float64) - ref.apply64(t, plain))
        bound = ref.matrix_bound(t, plain)
        print(f'yawed pose 150 m out: largest error {err.max():.3e} m, largest error / bound '
              f'{np.max(err / np.maximum(bound, 1e-300)):.3f}')
        assert (err <= bound).all()
        _assert_equal(got, ref.run_ref(c.host, c.prob, c.cos, c.sin, row_keep=c.host.row_keep, transforms=far))


def test_switch_gives_the_same_selection(case, monkeypatch):
    """the operator chain on the device (what OCOCC_OCC_FRAME_KERNEL=0 selects in OccDecoder.get_frame_occ): the same
    selection, flags, counts and -- without a matrix -- the same bits; with one, bmm's own rounding within the bound"""
    from objectcentricocccompletion_amd.occ import occ_base, occ_ops
    c = case
    _assert_equal(_run(occ_ops.occ_frame_select_aten, c, row_keep=c.row_keep), c.exp)
    _assert_equal(_run(occ_ops.occ_frame_select_aten, c, observed=False), ref.run_ref(c.host, c.prob, c.cos, c.sin, observed=False))
    far = torch.from_numpy(np.tile(ref.yawed_pose(0.7, 120.0, -90.0, 1.5), (c.R, 1)))
    got = _run(occ_ops.occ_frame_select_aten, c, row_keep=c.row_keep, transforms=far.to(c.logits.device))
    _assert_equal(got, c.exp, xyz=False)
    t = far.numpy()[np.repeat(np.arange(c.R), c.exp.counts)]
    err = np.abs(got[0][:, :3].cpu().numpy().astype(np.float64) - ref.apply64(t, c.exp.out[:, :3]))
    assert (err <= ref.matrix_bound(t, c.exp.out[:, :3])).all()
    # the decoder's dispatch: a stand-in decoder whose logits are the case's
    dec = occ_base.OccDecoder.__new__(occ_base.OccDecoder)
    torch.nn.Module.__init__(dec)
    dec.cls_dim, dec.pos_thresh = 1, c.pos_thresh
    dec.forward = lambda feats, centers, index: c.logits[:centers.size(0)].view(-1, 1)
    args = (torch.zeros(c.R, 4, device=c.logits.device), c.rois, ref.V, c.scale, c.offset, c.local_xyz, c.pts_roi)
    on = dec.get_frame_occ(*args, row_keep=c.row_keep)
    monkeypatch.setattr(occ_base, 'OCC_FRAME_KERNEL', False)
    monkeypatch.setattr(occ_ops, 'occ_frame_select', None)                               # the kernels are not reached
    off = dec.get_frame_occ(*args, row_keep=c.row_keep)
    _assert_equal(on, c.exp)
    _assert_equal(off, c.exp)


def test_without_rois_or_cells(dev):
    from objectcentricocccompletion_amd._lib import OcoccError
    from objectcentricocccompletion_amd.occ import occ_ops
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)
    e = occ_ops.dense_grid_layout(z(0, 3), ref.V)
    out, flags, counts = occ_ops.occ_frame_select(z(0), e[0], e[1], e[2], 0, ref.V, 0.5, z(0, 8), z(0, 3), z(0, dtype=torch.int32))
    assert tuple(out.shape) == (0, 4) and tuple(flags.shape) == (0,) and counts == []
    e = occ_ops.dense_grid_layout(z(3, 3), ref.V)                                         # three RoIs, none has a cell
    out, flags, counts = occ_ops.occ_frame_select(z(0), e[0], e[1], e[2], 0, ref.V, 0.5, z(3, 8), z(2, 3),
                                                  z(2, dtype=torch.int32))
    assert e[3] == 0 and tuple(out.shape) == (0, 4) and counts == [0, 0, 0]
    e = occ_ops.dense_grid_layout(torch.ones(2, 3, device=dev), ref.V)
    with pytest.raises(OcoccError, match=f'{e[3] - 1} logits for a layout of {e[3]} cells'):
        occ_ops.occ_frame_select(z(e[3] - 1), e[0], e[1], e[2], e[3], ref.V, 0.5, z(2, 8), z(0, 3), z(0, dtype=torch.int32))
    # a point whose RoI index is out of range marks nothing
    out, flags, counts = occ_ops.occ_frame_select(z(e[3]) - 5.0, e[0], e[1], e[2], e[3], ref.V, 0.5, z(2, 8), z(3, 3),
                                                  torch.tensor([0, 2, -1], dtype=torch.int32, device=dev))
    assert counts == [1, 0] and flags.tolist() == [2]
