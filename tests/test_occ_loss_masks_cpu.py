"""CPU suite: the sample masks of loss_occ's train_cfg variants -- occ_ops.occ_loss_masks_aten (what loss_occ takes on CPU
tensors and with OCOCC_OCC_LOSS_KERNEL=0, and the yardstick of csrc/occ_loss_masks.hip in
tests/test_gpu_occ_loss_masks.py) against the reference's lines restated literally (tests/occ_loss_masks_ref.py) on
crafted edges; the refusals of the kernel's wrapper and of the export; the export's declaration, binding and documents."""
import os
import re

import pytest
import torch

from occ_loss_masks_ref import EDGE_LOGITS, FLAG_SUBSETS, edge_case, reference_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'ococc_occ_loss_masks_f32'


def _both(case, pos_thresh, outside, observed, unmatched):
    from objectcentricocccompletion_amd.occ import occ_ops
    M, K = case['labels'].shape
    got = occ_ops.occ_loss_masks_aten(case['score'], case['score_thresh'], case['labels'].view(-1),
                                      xyz=case['xyz'].view(-1, 3), box_size=case['box_size'],
                                      ori_logits=case['ori_logits'].view(-1), pos_thresh=pos_thresh, outside=outside,
                                      observed=observed, unmatched=unmatched)
    exp = reference_lines(case['xyz'], case['box_size'], case['score'], case['ori_logits'].view(M, K, 1),
                          (case['labels'] == 1).long(), case['score_thresh'], pos_thresh, outside, observed, unmatched)
    return got, exp


@pytest.mark.parametrize('pos_thresh', [0.5, 0.3])
@pytest.mark.parametrize('outside,observed,unmatched', FLAG_SUBSETS)
def test_chain_equals_the_reference_lines_on_edges(pos_thresh, outside, observed, unmatched):
    case = edge_case()
    (w, um, counts), (ew, eum, ecounts) = _both(case, pos_thresh, outside, observed, unmatched)
    assert w.dtype == torch.float32 and torch.equal(w, ew)
    assert (um is None) == (not unmatched)
    if unmatched:
        assert um.dtype == torch.uint8 and torch.equal(um.bool(), eum)
    assert counts.dtype == torch.int64 and counts.tolist() == ecounts


def test_edges_decide_as_stated():
    """what the edge inputs are there for, asserted on the chain's own output"""
    case = edge_case()
    M, K = case['labels'].shape
    (w, um, counts), _ = _both(case, 0.5, True, False, True)
    w, um = w.view(M, K), um.view(M, K).bool()
    assert not w[1].any()                                    # a score equal to the threshold: weight 0
    kinds = ['on', 'beyond', 'nan'] * 12                     # the six (axis, sign) pairs in turn, twice; then interior points
    for k, kind in enumerate(kinds):
        assert bool(w[0, k]) == (kind == 'on') and bool(w[2, k]) == (kind == 'on'), (k, kind)
    assert w[0, len(kinds):].all() and w[2, len(kinds):].all()
    def ori_cls(pos_thresh):   # (RoI 0 is confident: its weight under `observed` alone is 0 where the class is 1)
        return _both(case, pos_thresh, False, True, False)[0][0].view(M, K)[0] == 0
    cls5, cls3 = ori_cls(0.5), ori_cls(0.3)
    for k in range(K):
        v = EDGE_LOGITS[k % len(EDGE_LOGITS)]
        if v != v:
            assert not cls5[k] and not cls3[k]               # NaN: class 0 under any threshold
        elif abs(v) >= 1e-6:
            assert bool(cls5[k]) == (v > 0)
        if v == v and abs(v) <= 1e-6:
            assert cls3[k]                                   # sigmoid ~ 0.5 > 0.3
        if v == float('-inf') or v == -88.0:
            assert not cls3[k]
    assert torch.equal(um[0], (case['labels'][0] == 1) != cls5)
    assert counts[1] == um.sum() and counts[2] == (um & (w > 0)).sum() and counts[0] == (w > 0).sum()


def test_empty_inputs():
    from objectcentricocccompletion_amd.occ import occ_ops
    for M, K in ((0, 8), (4, 0)):
        w, um, counts = occ_ops.occ_loss_masks_aten(torch.zeros(M), 0.4, torch.zeros(M * K, dtype=torch.int64),
                                                    xyz=torch.zeros(M * K, 3), box_size=torch.ones(M, 3),
                                                    ori_logits=torch.zeros(M * K), outside=True, observed=True, unmatched=True)
        assert w.shape == (0,) and um.shape == (0,) and counts.tolist() == [0, 0, 0]


def test_wrapper_refusals(monkeypatch):
    from objectcentricocccompletion_amd import _lib
    from objectcentricocccompletion_amd.occ import occ_ops
    M, K = 2, 3
    good = dict(score=torch.zeros(M), score_thresh=0.4, labels=torch.zeros(M * K, dtype=torch.int64),
                xyz=torch.zeros(M * K, 3), box_size=torch.ones(M, 3), ori_logits=torch.zeros(M * K), outside=True,
                observed=True, unmatched=True)
    with pytest.raises(_lib.OcoccError, match='CPU tensor'):
        occ_ops.occ_loss_masks(**good)
    # past the device check (a CPU tensor never reaches a launch: every case below is refused on its dtype or shape)
    monkeypatch.setattr(_lib, 'require_device', lambda *a, **k: None)
    bad = [dict(score=torch.zeros(M, dtype=torch.float64)), dict(labels=torch.zeros(M * K, dtype=torch.int32)),
           dict(labels=torch.zeros(M * K + 1, dtype=torch.int64)), dict(xyz=None), dict(xyz=torch.zeros(M * K, 2)),
           dict(xyz=torch.zeros(M * K, 3, dtype=torch.float16)), dict(box_size=torch.ones(M + 1, 3)), dict(box_size=None),
           dict(ori_logits=None), dict(ori_logits=torch.zeros(M * K, 2)), dict(ori_logits=torch.zeros(M * K).double()),
           dict(score=torch.zeros(0))]
    for change in bad:
        for fn in (occ_ops.occ_loss_masks, occ_ops.occ_loss_masks_aten):
            with pytest.raises(_lib.OcoccError):
                fn(**dict(good, **change))
    # inputs a switch does not read are not checked
    w, um, counts = occ_ops.occ_loss_masks_aten(**dict(good, xyz=None, box_size=None, ori_logits=None, outside=False,
                                                       observed=False, unmatched=False))
    assert w.tolist() == [0.0] * (M * K) and um is None and counts.tolist() == [0, 0, 0]


def test_export_is_declared_bound_and_documented():
    import ctypes
    from objectcentricocccompletion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ococc_hip.h')).read()
    m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % NAME, re.sub(r'/\*.*?\*/', '', header, flags=re.S))
    assert m, f'{NAME} is not declared in ococc_hip.h'
    assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[NAME][1]) == 14
    assert 'ococc_bbox_head.py:706-710' in header and ':713-722' in header     # the reference lines it replaces
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME) and hasattr(_lib.lib, NAME)
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert any(f'`{NAME}`' in line and line.startswith('|') for line in integration.splitlines()), 'no INTEGRATION.md row'
    assert 'occ_loss_masks.hip' in open(os.path.join(ROOT, 'objectcentricocccompletion_amd', 'csrc', 'Makefile')).read()
    assert 'OCOCC_OCC_LOSS_KERNEL' in open(os.path.join(ROOT, 'README.md')).read()
    assert _lib.lib.ococc_occ_loss_masks_pass_rows() > 0
    # invalid arguments are reported, not thrown, before anything is dereferenced or launched
    call = lambda M, K, flags: _lib.lib.ococc_occ_loss_masks_f32(None, None, None, None, None, M, K, 0.4, 0.5, flags, None,
                                                                 None, None, None)
    assert call(-1, 4, 0) == -1 and call(4, -1, 0) == -1
    assert call(1, 1, 8) == -1 and b'flags' in _lib.lib.ococc_last_error()
    assert call(1, 1, 7) == -1 and b'null pointer' in _lib.lib.ococc_last_error()
