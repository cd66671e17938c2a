"""occ_ops.occ_merge (csrc/occ_merge.hip) on the MI355X against its numpy restatement tests/occ_merge_ref.py: the bytes of
the whole output and the survivors per row, over the cell counts around the 1024-cell tile and the 4-tile block, rows
that are empty or straddle tiles, cloud sizes around the wave and the copy block, every use_dim form, scores at and next
to the threshold, NaN / inf / -0.0 / denormal scores, flag bytes with drop_observed on and off, and NaN and denormal
payload.  The operator chain occ_merge_aten gives the same bytes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_merge_ref as ref                                                   # noqa: E402

pytestmark = pytest.mark.gpu
CASES = ref.cases()


def _device(c, dev):
    t = lambda a, dt=None: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(points=t(c['points']), occ=t(c['occ']), counts=c['counts'], use_dim=c['use_dim'],
                row_score=t(c['row_score']), flags=t(c['flags']), drop_observed=c['drop_observed'],
                score_threshold=c['score_threshold'])


def _want(c):
    return ref.occ_merge_ref(c['points'], c['occ'], c['counts'], c['use_dim'], c['row_score'], c['flags'],
                             c['drop_observed'], c['score_threshold'])


def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_merge_equals_the_restatement(c, dev):
    from objectcentricocccompletion_amd.occ import occ_ops
    want, want_counts = _want(c)
    args = _device(c, dev)
    got, counts = occ_ops.occ_merge(**args)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_contiguous()
    assert isinstance(counts, list) and counts == want_counts
    assert _bytes(got) == want.tobytes()
    chain, chain_counts = occ_ops.occ_merge_aten(**args)
    assert chain_counts == want_counts and _bytes(chain) == want.tobytes()
    again, _ = occ_ops.occ_merge(**args)
    assert _bytes(again) == _bytes(got)


def test_everything_kept_is_occ_itself(dev):
    """threshold -inf, no flags, use_dim (0, 1, 2): the tail is occ's own xyz and value columns, bit for bit"""
    from objectcentricocccompletion_amd.occ import occ_ops
    c = ref.case('tail', 130, ref.STRADDLE, use_dim=(0, 1, 2), threshold=-np.inf, seed=41)
    c['occ'][5, 3] = np.inf
    keep = ~np.isnan(c['occ'][:, 3])                         # (a NaN value is not > -inf)
    got, counts = occ_ops.occ_merge(**_device(c, dev))
    got = got.cpu().numpy()
    assert got.shape == (130 + keep.sum(), 5)
    assert got[130:, :3].tobytes() == c['occ'][keep][:, :3].tobytes()
    assert got[130:, 3].tobytes() == c['occ'][keep][:, 3].tobytes() and (got[130:, 4] == 1).all()
    assert got[:130, :3].tobytes() == c['points'][:, :3].tobytes() and (got[:130, 3:] == 0).all()
    assert sum(counts) == keep.sum()


def test_operator_refuses_on_the_device(dev):
    """the refusals that need device tensors to get past the CPU check"""
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ import occ_ops
    pts, occ = torch.zeros(4, 6, device=dev), torch.zeros(5, 4, device=dev)
    with pytest.raises(L.OcoccError, match='use_dim'):
        occ_ops.occ_merge(pts, occ, [5], use_dim=(0, 1, 6))
    with pytest.raises(L.OcoccError, match='sum'):
        occ_ops.occ_merge(pts, occ, [2, 2])
    with pytest.raises(L.OcoccError, match='CPU tensor'):
        occ_ops.occ_merge(pts, occ, [5], flags=torch.zeros(5, dtype=torch.uint8), drop_observed=True)
