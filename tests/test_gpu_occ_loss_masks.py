"""GPU suite: csrc/occ_loss_masks.hip (ococc_occ_loss_masks_f32 behind occ_ops.occ_loss_masks) against the reference's
operator chain on the same device (occ_ops.occ_loss_masks_aten, pinned to the reference's lines by
tests/test_occ_loss_masks_cpu.py): weights, unmatched bytes and the three counts BIT-EQUAL, for every subset of the three
flags, at the shapes where the kernel takes another path:

  (1, 1)        one row: the ragged group of four only
  (5, 70)       350 rows: a ragged second workgroup, waves and groups of four rows that straddle two RoIs
  (3, 512)      whole groups only
  (0, 8) (4, 0) no launch, counts zero
  (3, 43691)    2^17 + 1 rows: one row past what a single pass of the capped grid covers (the grid-stride trip)
  misaligned    the same rows from views one element into their buffers: the element-wise loads and stores"""
import pytest
import torch

from occ_loss_masks_ref import FLAG_SUBSETS, edge_case

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 70), (3, 512), (3, 43691)]
SCORE_THRESH, POS_THRESH = 0.4, 0.5


def _inputs(M, K, dev, seed=0):
    """samples around their boxes' faces (some exactly on one), logits around 0 with NaN / inf sprinkled in, labels in
    {0, 1, 2}, label confidences around the threshold (one equal to it)"""
    g = torch.Generator().manual_seed(seed + 1000 * M + K)
    size = torch.rand(M, 3, generator=g) * torch.tensor([1.0, 3.0, 0.8]) + torch.tensor([1.6, 3.5, 1.2])
    xyz = (torch.rand(M, K, 3, generator=g) - 0.5) * size[:, None, :] * 1.3
    on_face = torch.rand(M, K, generator=g) < 0.05
    axis = torch.randint(0, 3, (M, K), generator=g)
    sign = torch.randint(0, 2, (M, K), generator=g).float() * 2 - 1
    face = (size / 2)[torch.arange(M)[:, None].expand(M, K), axis] * sign
    for a in range(3):
        xyz[..., a][on_face & (axis == a)] = face[on_face & (axis == a)]
    xyz[torch.rand(M, K, generator=g) < 0.01] = float('nan')
    logits = torch.randn(M, K, generator=g) * 2
    near = torch.rand(M, K, generator=g) < 0.1
    logits[near] = (torch.randint(-4, 5, (M, K), generator=g).float() * 3e-8)[near]
    logits[torch.rand(M, K, generator=g) < 0.01] = float('nan')
    logits[torch.rand(M, K, generator=g) < 0.01] = float('inf')
    labels = torch.randint(0, 3, (M, K), generator=g)
    score = torch.rand(M, generator=g) * 0.4 + 0.3
    score[0] = 0.9
    if M > 2:
        score[1] = SCORE_THRESH
    return dict(xyz=xyz.view(-1, 3).to(dev), box_size=size.to(dev), score=score.to(dev), ori_logits=logits.view(-1).to(dev),
                labels=labels.view(-1).to(dev))


def _run(fn, case, outside, observed, unmatched, score_thresh=SCORE_THRESH, pos_thresh=POS_THRESH):
    return fn(case['score'], score_thresh, case['labels'].reshape(-1), xyz=case['xyz'].reshape(-1, 3),
              box_size=case['box_size'], ori_logits=case['ori_logits'].reshape(-1), pos_thresh=pos_thresh, outside=outside,
              observed=observed, unmatched=unmatched)


def _assert_equal(got, exp):
    (w, um, counts), (ew, eum, ecounts) = got, exp
    assert w.dtype == torch.float32 and w.shape == ew.shape and torch.equal(w, ew)
    assert (um is None) == (eum is None)
    if um is not None:
        assert um.dtype == torch.uint8 and torch.equal(um, eum)
    assert counts.dtype == torch.int64 and torch.equal(counts, ecounts), (counts.tolist(), ecounts.tolist())


@pytest.fixture(scope='module')
def cases(dev):
    return {shape: _inputs(*shape, dev) for shape in SHAPES}


@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_equals_chain_bit_for_bit(dev, cases, shape):
    from objectcentricocccompletion_amd import _lib
    from objectcentricocccompletion_amd.occ import occ_ops
    if shape == SHAPES[-1]:
        assert shape[0] * shape[1] == _lib.lib.ococc_occ_loss_masks_pass_rows() + 1
    case = cases[shape]
    for flags in FLAG_SUBSETS:
        got = _run(occ_ops.occ_loss_masks, case, *flags)
        _assert_equal(got, _run(occ_ops.occ_loss_masks_aten, case, *flags))
        again = _run(occ_ops.occ_loss_masks, case, *flags)          # integer counts: two runs, equal bits
        _assert_equal(again, got)
    w, um, counts = _run(occ_ops.occ_loss_masks, case, True, True, True)
    if shape[0] * shape[1] >= 350:   # the inputs exercise what they claim to
        assert 0 < counts[2] < counts[1] < w.numel() and 0 < counts[0] < w.numel()


@pytest.mark.parametrize('shape', [(0, 8), (4, 0)])
def test_empty_shapes_launch_nothing(dev, shape):
    from objectcentricocccompletion_amd.occ import occ_ops
    M, K = shape
    case = dict(xyz=torch.zeros(M * K, 3, device=dev), box_size=torch.ones(M, 3, device=dev), score=torch.ones(M, device=dev),
                ori_logits=torch.zeros(M * K, device=dev), labels=torch.zeros(M * K, dtype=torch.int64, device=dev))
    for flags in FLAG_SUBSETS:
        w, um, counts = _run(occ_ops.occ_loss_masks, case, *flags)
        assert w.shape == (0,) and (um is None or um.shape == (0,)) and counts.tolist() == [0, 0, 0]
        _assert_equal((w, um, counts), _run(occ_ops.occ_loss_masks_aten, case, *flags))


@pytest.mark.parametrize('pos_thresh', [0.5, 0.3])
def test_edge_values(dev, pos_thresh):
    """the CPU test's crafted edges: coordinates on +-size / 2, one ulp beyond and NaN; logits 0, +-1e-8 ... +-inf, NaN;
    a score equal to the threshold"""
    from objectcentricocccompletion_amd.occ import occ_ops
    case = edge_case(dev)
    thr = case.pop('score_thresh')
    for flags in FLAG_SUBSETS:
        got = _run(occ_ops.occ_loss_masks, case, *flags, score_thresh=thr, pos_thresh=pos_thresh)
        _assert_equal(got, _run(occ_ops.occ_loss_masks_aten, case, *flags, score_thresh=thr, pos_thresh=pos_thresh))
    M, K = case['labels'].shape
    w = _run(occ_ops.occ_loss_masks, case, True, False, False, score_thresh=thr)[0].view(M, K)
    assert not w[1].any()                                                     # score == threshold
    assert w[0, :36].view(12, 3).t().tolist() == [[1.0] * 12, [0.0] * 12, [0.0] * 12]   # on / one ulp beyond / NaN


def test_only_the_inputs_of_the_flags_are_read(dev, cases):
    """no ori_logits with only the outside flag; no xyz / box_size with only the logit flags"""
    from objectcentricocccompletion_amd.occ import occ_ops
    case = cases[(5, 70)]
    for fn_flags, drop in (((True, False, False), ('ori_logits',)), ((False, True, True), ('xyz', 'box_size')),
                           ((False, False, False), ('xyz', 'box_size', 'ori_logits'))):
        part = dict(case, **{k: None for k in drop})
        call = lambda fn, c: fn(c['score'], SCORE_THRESH, c['labels'], xyz=c['xyz'], box_size=c['box_size'],
                                ori_logits=c['ori_logits'], pos_thresh=POS_THRESH, outside=fn_flags[0], observed=fn_flags[1],
                                unmatched=fn_flags[2])
        _assert_equal(call(occ_ops.occ_loss_masks, part), call(occ_ops.occ_loss_masks_aten, case))


def test_misaligned_views_take_the_element_wise_path(dev, cases):
    from objectcentricocccompletion_amd.occ import occ_ops
    case = cases[(5, 70)]
    M, K = 5, 70

    def shifted(t, by):   # the same values, `by` elements into a fresh buffer: contiguous, not 16-byte aligned
        buf = torch.empty(t.numel() + by, dtype=t.dtype, device=dev)
        buf[by:] = t.reshape(-1)
        return buf[by:].view(t.shape)

    off = dict(case, xyz=shifted(case['xyz'], 1), ori_logits=shifted(case['ori_logits'], 3), labels=shifted(case['labels'], 1))
    assert off['xyz'].data_ptr() % 16 and off['ori_logits'].data_ptr() % 16 and off['labels'].data_ptr() % 16
    for flags in FLAG_SUBSETS:
        _assert_equal(_run(occ_ops.occ_loss_masks, off, *flags), _run(occ_ops.occ_loss_masks_aten, case, *flags))


def test_wrapper_refuses_before_any_launch(dev, cases):
    from objectcentricocccompletion_amd import _lib
    from objectcentricocccompletion_amd.occ import occ_ops
    case = cases[(5, 70)]
    for change in (dict(score=case['score'].cpu()), dict(labels=case['labels'].int()), dict(xyz=case['xyz'][:-1]),
                   dict(ori_logits=case['ori_logits'].double()), dict(box_size=case['box_size'][:2])):
        with pytest.raises(_lib.OcoccError):
            _run(occ_ops.occ_loss_masks, dict(case, **change), True, True, True)
