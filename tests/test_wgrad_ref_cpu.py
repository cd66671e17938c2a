"""tests/wgrad_ref.py, the float64 reference and the case table the weight-gradient kernel tests use
(tests/test_gpu_wgrad_edges.py): the reference against the CPU oracle on a real sub-manifold rulebook, the exactness
condition of every case, and every case against the partition edge it is meant to hit -- through the Python restatement
of the partition formulas, whose constants are compared with csrc/sparse_conv.hip as text.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_ref as R        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'objectcentricocccompletion_amd', 'csrc', 'sparse_conv.hip')


def _source():
    with open(SOURCE) as f:
        return f.read()


def test_wgrad_f64_equals_the_oracle_on_a_submanifold_rulebook():
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    B, shape = 2, (6, 7, 8)
    mask = rng.random((B,) + shape) < 0.35
    idx = np.argwhere(mask).astype(np.int32)
    idx = idx[rng.permutation(len(idx))]
    n, cin, cout = len(idx), 5, 7
    pairs, num = O.subm_rulebook(idx, B, shape)
    assert num[13] == n and int(num.sum()) > 3 * n and int(num.min()) > 0     # a rulebook with every offset in use
    x = rng.integers(-3, 4, (n, cin)).astype(np.float32)         # integers: the oracle's float32 sums are exact too
    dy = rng.integers(-3, 4, (n, cout)).astype(np.float32)
    w = np.zeros((3, 3, 3, cin, cout), np.float32)
    _, edw = O.indice_conv_backward(x, w, dy, pairs, num, subm=True)
    got = R.wgrad_f64(torch.from_numpy(x), torch.from_numpy(dy), torch.from_numpy(pairs), torch.from_numpy(num))
    assert got.dtype == torch.float64 and tuple(got.shape) == (27, cin, cout)
    assert torch.equal(got, torch.from_numpy(edw.reshape(27, cin, cout)).double())
    # ... and it reads no pair behind num[k]: other valid rows there change nothing
    filled = torch.from_numpy(pairs).clone()
    for k in range(27):
        filled[k, :, num[k]:] = torch.randint(0, n, (2, n - int(num[k])), dtype=torch.int32)
    assert torch.equal(R.wgrad_f64(torch.from_numpy(x), torch.from_numpy(dy), filled, torch.from_numpy(num)), got)
    absolute = R.wgrad_f64(torch.from_numpy(x), torch.from_numpy(dy), filled, torch.from_numpy(num), absolute=True)
    assert bool((absolute >= got.abs()).all())


def test_make_case_fills_the_tails_with_rows_that_are_not_the_list():
    num = [0, 5, 40, 17]
    x, dy, pairs, nt = R.make_case(num, 40, 12, 9, 16, 32, seed=3)
    assert x.dtype == dy.dtype == torch.bfloat16 and pairs.dtype == nt.dtype == torch.int32
    assert tuple(x.shape) == (12, 16) and tuple(dy.shape) == (9, 32) and tuple(pairs.shape) == (4, 2, 40) and nt.tolist() == num
    assert pairs.is_contiguous()
    assert int(pairs[:, 0].min()) >= 0 and int(pairs[:, 0].max()) < 12 and int(pairs[:, 1].min()) >= 0 and int(pairs[:, 1].max()) < 9
    assert bool((pairs[:, 0] != pairs[:, 1]).all()), 'the two rows of a pair differ'
    assert set(x.float().unique().tolist()) <= set(range(-3, 4)) and x.float().abs().max() == 3
    ref = R.wgrad_f64(x, dy, pairs, nt)
    assert float(ref[0].abs().max()) == 0 and float(ref[1].abs().max()) > 0
    longer = nt.clone()
    longer[1] = 6       # one pair of the tail read as if it belonged to the list: another sum
    assert not torch.equal(R.wgrad_f64(x, dy, pairs, longer)[1], ref[1])
    again = R.make_case(num, 40, 12, 9, 16, 32, seed=3)
    assert all(torch.equal(a, b) for a, b in zip(again, (x, dy, pairs, nt)))
    xn = R.make_case(num, 40, 12, 9, 16, 32, seed=3, values='normal')[0]
    assert xn.dtype == torch.bfloat16 and len(xn.float().unique()) > 50


def test_every_case_is_exact_in_float32():
    """9 * num[k] < 2^24: every partial sum of products of integers in -3..3 is an exactly represented integer"""
    worst = 0
    for name, num in R.all_nums():
        assert 9 * max(num) < R.EXACT_LIMIT, f'{name}: 9 * {max(num)} reaches 2^24, the sums are no longer exact'
        worst = max(worst, max(num))
    assert worst == 262656
    for rows, c in R.LN_TABLES:
        assert 3 * rows < R.EXACT_LIMIT


def test_constants_are_those_of_the_source():
    """the table is laid out around these numbers: when one changes in the kernel file the cases have to move with it"""
    src = _source()
    for name, mine in (('kWgSteps', R.K_WG_STEPS), ('kWgGrid', R.K_WG_GRID), ('kWgDepth', R.K_WG_DEPTH),
                       ('kReduceGrid', R.K_REDUCE_GRID), ('kMaxReduce', R.MAX_REDUCE)):
        m = re.findall(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, src)
        assert len(m) == 1, f'{name}: {len(m)} definitions found in sparse_conv.hip'
        assert int(m[0]) == mine, f'{name} is {m[0]} in sparse_conv.hip and {mine} in wgrad_ref.py: re-derive the case table'
    # the rule of the joint reduction and the share of a job of the shared launch, as the source spells them
    assert re.search(r'my_slabs\s*>\s*%d\s*\?\s*deep_units\s*:\s*wide_units' % R.WIDE_SLABS, src), 'wide/deep rule moved'
    assert re.search(r'nsl\s*<=\s*%d\b' % R.WIDE_SLABS, src), 'wide/deep rule moved'
    assert re.search(r'maxg\s*<\s*kWgGrid\s*/\s*4\s*\?\s*maxg\s*:\s*kWgGrid\s*/\s*4', src), 'share of a shared-launch job moved'
    assert re.search(r'constexpr\s+int\s+U\s*=\s*16\s*;', src), 'the deep sum is no longer 16-way unrolled'


def test_step_counts_land_on_their_edges():
    assert len(R.STEP_NUM) == 27 and R.STEP_CAP > max(R.STEP_NUM)
    for n, (st, it, last) in R.STEP_COUNTS.items():
        assert n in R.STEP_NUM, f'count {n} has no offset'
        assert R.steps(n) == st, f'count {n}: {R.steps(n)} steps, meant {st}'
        assert R.items(n) == it, f'count {n}: {R.items(n)} work items, meant {it}'
        if n:
            assert R.last_item_steps(n) == last, f'count {n}: last item of {R.last_item_steps(n)} steps, meant {last}'
    D, S = R.K_WG_DEPTH, R.K_WG_STEPS
    assert [R.steps(n) for n in (96, 128, 129, 160)] == [D - 1, D, D + 1, D + 1], 'the counts around the register ring'
    assert R.steps(512) == S and R.steps(513) == S + 1 and R.steps(545) == S + 2 and R.steps(1024) == 2 * S
    assert R.items(32 * S) == 1 and R.items(32 * S + 1) == 2 and R.items(64 * S) == 2 and R.items(64 * S + 1) == 3
    # slabs_before: the running sum of the items
    assert R.slabs_before(R.STEP_NUM, 0) == 0 and R.slabs_before(R.STEP_NUM, 1) == 2 and R.slabs_before(R.STEP_NUM, 4) == 6
    assert R.total_items(R.STEP_NUM) == sum(R.items(n) for n in R.STEP_NUM) <= R.max_groups(27, R.STEP_CAP)
    assert R.total_items(R.STEP_NUM) < R.single_grid(27, R.STEP_CAP), 'this case is not meant to loop over items'


@pytest.mark.parametrize('name', sorted(R.REDUCE_CASES))
def test_reduce_cases_land_on_their_edges(name):
    c = R.REDUCE_CASES[name]
    num, cap = c['num'], max(c['num'])
    assert len(num) == 4
    got = [R.items(n) for n in num]
    assert got == c['slabs'], f'{name} ({c["why"]}): slabs per offset {got}, meant {c["slabs"]}'
    for cin, cout in (R.REDUCE_SMALL, R.REDUCE_BIG):
        units = R.reduce_units(num, cin * cout)
        assert [kind == 'deep' for kind, _ in units] == c['deep'], f'{name}: deep offsets {units}, meant {c["deep"]}'
        assert all(u == (cin * cout // 16 if kind == 'deep' else cin * cout // 256) for kind, u in units)
    assert R.total_items(num) <= R.max_groups(4, cap) and R.total_items(num) < R.single_grid(4, cap)
    assert [R.slabs_before(num, k) for k in range(4)] == [sum(c['slabs'][:k]) for k in range(4)]


def test_reduce_cases_cover_every_edge_of_the_two_sums():
    slabs = {s: c['deep'][i] for c in R.REDUCE_CASES.values() for i, s in enumerate(c['slabs'])}
    W = R.WIDE_SLABS
    for s in (W // 2, W // 2 + 1, W, W + 1, 240, 241, 256, 257, 513):
        assert s in slabs, f'no offset with {s} slabs'
        assert slabs[s] == (s > W), f'{s} slabs on the wrong side of the wide/deep rule'
    # the unrolled loop of the deep sum runs while lane + 16 * 15 < slabs, in strides of 16 * 16
    assert 16 * 15 == 240 and 16 * 16 == 256
    big = R.REDUCE_CASES['big_16_17_256_257']
    assert set(big['slabs']) == {W, W + 1, 256, 257}
    # a deep offset directly behind an empty one and behind a one-slab one
    behind = {(c['slabs'][i - 1], c['deep'][i]) for c in R.REDUCE_CASES.values() for i in range(1, 4)}
    assert (0, True) in behind and (1, True) in behind
    dense = R.REDUCE_CASES['deep_513']
    assert max(dense['num']) == 262656 == 513 * 512 == max(max(c['num']) for c in R.REDUCE_CASES.values())


@pytest.mark.parametrize('key', sorted(R.WAVE_CASES))
def test_wave_cases_land_in_their_chunk(key):
    kvol, pattern = key
    c = R.WAVE_CASES[key]
    num = c['num']
    assert len(num) == kvol and max(num) <= R.WAVE_CAP and R.total_items(num) >= 1
    assert R.first_chunk(num) == c['chunk'], f'{key}: the first item lies in chunk {R.first_chunk(num)}, meant {c["chunk"]}'
    if pattern == 'late' and kvol > 64:
        assert not any(num[:64]) and num[64] > 0 and c['chunk'] == 1
    if pattern == 'marks':
        for k in (0, 63, 64, kvol - 1):
            assert k >= kvol or num[k] > 0, f'{key}: offset {k} is empty'
    units = R.reduce_units(num, 32 * 16)
    if kvol > 64:   # the division branch: every offset deep, empty ones included, more units than the grid
        assert all(kind == 'deep' for kind, _ in units) and 0 in num
        if kvol >= 125:
            assert sum(u for _, u in units) > R.K_REDUCE_GRID
    else:
        assert all(kind == 'wide' for kind, _ in units)
    assert R.total_items(num) <= R.max_groups(kvol, R.WAVE_CAP)


def test_wave_cases_cover_both_branches():
    assert set(k for k, _ in R.WAVE_CASES) == {1, 63, 64, 65, 125, 129}
    assert sorted(k for k, _ in R.WAVE_CASES if k <= 64) == [1, 1, 63, 63, 64, 64]
    assert [R.WAVE_CASES[(k, 'late')]['chunk'] for k in (65, 125, 129)] == [1, 1, 1]
    assert R.first_chunk(R.wave_num(129, 'late')) == 1 and R.wave_num(129, 'marks')[128] > 0


@pytest.mark.parametrize('which', ['loop_single', 'loop_shared'])
def test_loop_cases_are_longer_than_their_grid(which):
    c = R.CASES[which]
    num, kvol, cap = c['num'], c['kvol'], c['cap']
    grid = R.single_grid(kvol, cap) if which == 'loop_single' else R.shared_grid(kvol, cap)
    assert grid == c['grid'] == (R.K_WG_GRID if which == 'loop_single' else R.K_WG_GRID // 4), f'{which}: grid {grid}'
    assert all(R.items(n) == c['items_per_offset'] for n in num)
    assert R.total_items(num) == c['items'] > grid, f'{which}: {R.total_items(num)} items do not exceed the grid {grid}'
    assert R.total_items(num) <= R.max_groups(kvol, cap), 'the workspace holds every slab'
    assert R.total_items(num) < 2 * grid, 'one extra trip, for a few workgroups'
    assert R.second_trip(num, grid) == c['second'], f'{which} ({c["why"]}): second trip {R.second_trip(num, grid)}'
    if which == 'loop_shared':
        assert R.last_item_steps(num[26]) == 1 and num[26] % 32 == 1
        assert (c['cin'], c['cout']) in R.SHARED_SHAPES


def test_shared_jobs_and_the_eight():
    for order in R.SHARED_ORDERS:
        assert 2 <= len(order) <= 3
    assert {(2 in o) for o in R.SHARED_ORDERS} == {True, False}     # both instantiations of the shared launch
    assert (2, 1, 0) in R.SHARED_ORDERS and (0, 1, 2) in R.SHARED_ORDERS
    kv = [len(j['num']) for j in R.SHARED_JOBS]
    assert len(set(kv)) == 3 and len({j['cap'] for j in R.SHARED_JOBS}) == 3
    last = R.SHARED_JOBS[1]['num']
    assert not any(last[:-1]) and R.items(last[-1]) == 2, 'a job whose items are all in its last offset'
    assert R.first_chunk(R.SHARED_JOBS[2]['num']) == 0 and R.SHARED_JOBS[2]['num'][64] > 0
    for j in R.SHARED_JOBS:
        assert max(j['num']) <= j['cap'] and R.total_items(j['num']) < R.shared_grid(len(j['num']), j['cap'])
    assert len(R.EIGHT) == R.MAX_REDUCE
    kinds, total = set(), 0
    for j in R.EIGHT:
        assert max(j['num']) <= j['cap'] and j['cin'] in R.CHANNELS and j['cout'] in R.CHANNELS
        units = R.reduce_units(j['num'], j['cin'] * j['cout'])
        kinds |= {(len(j['num']) > 64, kind) for kind, _ in units}
        total += sum(u for _, u in units)
    assert kinds == {(False, 'wide'), (False, 'deep'), (True, 'deep')}
    assert {len(j['num']) for j in R.EIGHT} >= {27, 125}
    assert total > R.K_REDUCE_GRID, 'the eight reductions make the fixed grid walk its unit list more than once'
    assert any(rows > 32 * 31 for rows, _ in R.LN_TABLES) and any(rows == 1 for rows, _ in R.LN_TABLES)
