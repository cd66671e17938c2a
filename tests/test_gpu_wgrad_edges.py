"""The weight-gradient kernels of the sparse convolution (csrc/sparse_conv.hip: wgrad_kernel<CIN, COUT>,
wgrad_pair_kernel<BIG>, wgrad_reduce_kernel, wgrad_reduce_multi_kernel, backward_reduce_multi_kernel) against the float64
contraction of tests/wgrad_ref.py, through the C entry points (no routing of spconv/ops.py in between), with pair lists
written by hand at the counts where the partition into steps, work items, slabs and reduction units changes.

Every case but the last draws x and dy as integers in -3..3: all partial sums are exactly represented integers (the
condition is checked per case in tests/test_wgrad_ref_cpu.py), so dW has to equal the float64 result bit for bit in any
summation order, and nothing here is a tolerance.  In every case the tails of the pair lists hold valid rows that do not
belong to the list, the workspace and dW are filled with NaN before each call, and a second call has to give the same
bits.  The last case (normal values) is held to a derived bound and prints 'WGRADEDGE ... error / bound'; measured on
gfx950 when this file was written: 1.4e-5 (wgrad_reduce_kernel), 1.1e-5 (the joint reduction); worst error 5.4e-4."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_ref as R        # noqa: E402

pytestmark = pytest.mark.gpu

N_ROWS = 192          # feature rows: the pair lists, not the features, carry the size
EINVAL, EUNSUPPORTED = -1, -3


@pytest.fixture(scope='module')
def L():
    from objectcentricocccompletion_amd import _lib
    return _lib


class Job(object):
    """one weight-gradient problem on the device: operands, its float64 result, NaN-filled workspace and dW"""

    def __init__(self, L, dev, num, cap, cin, cout, seed, values='int'):
        x, dy, pairs, nt = R.make_case(num, cap, N_ROWS, N_ROWS, cin, cout, seed, values)
        self.x, self.dy, self.pairs, self.num = x.to(dev), dy.to(dev), pairs.to(dev), nt.to(dev)
        self.kvol, self.cap, self.cin, self.cout, self.counts = len(num), cap, cin, cout, list(num)
        self.ref = R.wgrad_f64(self.x, self.dy, self.pairs, self.num)
        nbytes = int(L.lib.ococc_sparse_conv_wgrad_workspace_bytes(self.kvol, cap, cin, cout))
        assert nbytes == R.workspace_bytes(self.kvol, cap, cin, cout)
        self.ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        self.dw = torch.empty(self.kvol, cin, cout, dtype=torch.float32, device=dev)
        self.poison()

    def poison(self):
        self.ws.fill_(float('nan'))
        self.dw.fill_(float('nan'))

    def slabs(self, L, reduce):
        """ococc_sparse_conv_wgrad_bf16: slabs, and with reduce the sums of wgrad_reduce_kernel in dw"""
        rc = L.lib.ococc_sparse_conv_wgrad_bf16(self.x.data_ptr(), N_ROWS, self.cin, self.dy.data_ptr(), N_ROWS, self.cout,
                                                self.pairs.data_ptr(), self.num.data_ptr(), self.kvol, self.cap,
                                                self.dw.data_ptr() if reduce else None, self.ws.data_ptr(),
                                                self.ws.numel() * 4, L.stream())
        assert rc == 0, L.lib.ococc_last_error()


def _tables(n):
    return ctypes.c_void_p * n, ctypes.c_int32 * n, ctypes.c_int64 * n


def _shared_launch(L, jobs):
    """ococc_sparse_conv_wgrad_multi_bf16 -> return code"""
    vp, i32, i64 = _tables(len(jobs))
    return L.lib.ococc_sparse_conv_wgrad_multi_bf16(
        len(jobs), vp(*[j.x.data_ptr() for j in jobs]), vp(*[j.dy.data_ptr() for j in jobs]), i32(*[j.cin for j in jobs]),
        i32(*[j.cout for j in jobs]), vp(*[j.pairs.data_ptr() for j in jobs]), vp(*[j.num.data_ptr() for j in jobs]),
        i32(*[j.kvol for j in jobs]), i64(*[j.cap for j in jobs]), vp(*[j.ws.data_ptr() for j in jobs]),
        i64(*[j.ws.numel() * 4 for j in jobs]), L.stream())


def _reduce_args(jobs):
    vp, i32, i64 = _tables(len(jobs))
    return (len(jobs), vp(*[j.ws.data_ptr() for j in jobs]), vp(*[j.num.data_ptr() for j in jobs]),
            i32(*[j.kvol for j in jobs]), i64(*[j.cin * j.cout for j in jobs]), vp(*[j.dw.data_ptr() for j in jobs]))


def _joint_reduce(L, jobs):
    """ococc_sparse_conv_wgrad_reduce_multi -> return code"""
    return L.lib.ococc_sparse_conv_wgrad_reduce_multi(*_reduce_args(jobs), L.stream())


def _exact(what, job, offsets=None):
    """dW of the job equals the float64 contraction bit for bit (NaN fails); names the offsets that do not"""
    got = job.dw.double()
    ks = range(job.kvol) if offsets is None else offsets
    bad = [k for k in ks if not torch.equal(got[k], job.ref[k])]
    if bad:
        k = bad[0]
        diff = (got[k] != job.ref[k]) | got[k].isnan()
        i = int(diff.flatten().nonzero()[0])
        raise AssertionError(
            f'{what}: dW differs from float64 at offsets {bad[:12]}{"..." if len(bad) > 12 else ""} '
            f'(pairs {[job.counts[b] for b in bad[:12]]}, slabs {[R.items(job.counts[b]) for b in bad[:12]]}); offset {k}: '
            f'{int(diff.sum())} of {diff.numel()} elements, first at {divmod(i, job.cout)}: got {float(got[k].flatten()[i])}, '
            f'float64 {float(job.ref[k].flatten()[i])}')


def _twice(what, jobs, run, offsets=None):
    """run() fills dw of every job from poisoned buffers: twice the same bits, and those of float64"""
    first = []
    for attempt in range(2):
        for j in jobs:
            j.poison()
        run()
        torch.cuda.synchronize()
        if attempt == 0:
            first = [j.dw.clone() for j in jobs]
    for i, j in enumerate(jobs):
        _exact(f'{what}, job {i} ({j.cin} x {j.cout}, kvol {j.kvol})', j, offsets)
        assert torch.equal(first[i], j.dw), f'{what}, job {i}: two calls gave different bits'


def _single_both_reductions(what, L, job, offsets=None):
    """the single launch, finished by wgrad_reduce_kernel and by the joint reduction"""
    _twice(what + ' / wgrad_reduce_kernel', [job], lambda: job.slabs(L, True), offsets)

    def later():
        job.slabs(L, False)
        assert _joint_reduce(L, [job]) == 0, L.lib.ococc_last_error()
    _twice(what + ' / wgrad_reduce_multi_kernel', [job], later, offsets)


# ---- (a) step, ring and item edges, every instantiation --------------------------------------------------------------
@pytest.mark.parametrize('cout', R.CHANNELS)
@pytest.mark.parametrize('cin', R.CHANNELS)
def test_step_ring_and_item_edges(dev, L, cin, cout):
    """one offset per count of R.STEP_COUNTS (0, one pair, around one step, around the register ring of four steps,
    around one and two work items), in each of the 16 wgrad_kernel<CIN, COUT>"""
    job = Job(L, dev, R.STEP_NUM, R.STEP_CAP, cin, cout, seed=100 * cin + cout)
    assert float(job.ref[R.STEP_NUM.index(0)].abs().max()) == 0 and float(job.ref[R.STEP_NUM.index(1)].abs().max()) > 0
    _single_both_reductions(f'steps {cin} x {cout}', L, job)


# ---- (b) reduction edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['wide_8_9_16_17', 'deep_after_empty', 'deep_after_one_slab', 'deep_513'])
def test_reduction_edges(dev, L, name):
    """slabs per offset at 8|9 (second half of the wide sum), 16|17 (wide|deep), 240|241, 256|257 and 513 (the unrolled
    loop of the deep sum); deep offsets behind an empty and behind a one-slab offset (their first slab)"""
    c = R.REDUCE_CASES[name]
    job = Job(L, dev, c['num'], max(c['num']), *R.REDUCE_SMALL, seed=len(name))
    _single_both_reductions(f'{name} ({c["why"]})', L, job)


def test_reduction_edges_at_64x128(dev, L):
    c = R.REDUCE_CASES['big_16_17_256_257']
    job = Job(L, dev, c['num'], max(c['num']), *R.REDUCE_BIG, seed=7)
    _single_both_reductions(f'big_16_17_256_257 ({c["why"]})', L, job)


# ---- (c) offsets beyond one wave -------------------------------------------------------------------------------------
@pytest.mark.parametrize('pattern', ['late', 'marks'])
@pytest.mark.parametrize('kvol', R.WAVE_KVOLS)
def test_offsets_beyond_one_wave(dev, L, kvol, pattern):
    """'late' above 64 offsets: the first work item lies in the second 64-offset chunk of wg_locate; 'marks': pairs at
    offsets 0, 63, 64, kvol - 1.  Up to 64 offsets the joint reduction finds its units by a wave scan, above by division
    (every offset summed deep, the empty ones too: they have to come out as zeros)"""
    c = R.WAVE_CASES[(kvol, pattern)]
    job = Job(L, dev, c['num'], R.WAVE_CAP, 32, 16, seed=kvol)
    _single_both_reductions(f'kvol {kvol} {pattern}', L, job)


# ---- (d) work lists longer than the grid ------------------------------------------------------------------------------
def test_single_launch_loops_over_items(dev, L):
    """27 x 79 = 2 133 work items on 2 048 workgroups: items 2 048 .. 2 132 -- the last six of offset 25 and all 79 of
    offset 26 -- are reached by the item += item_stride trip of workgroups 0 .. 84"""
    c = R.LOOP_SINGLE
    job = Job(L, dev, c['num'], c['cap'], c['cin'], c['cout'], seed=11)
    second = sorted(c['second'])
    assert second == [25, 26]
    _twice('second trip of the single launch (offsets 25, 26)', [job], lambda: job.slabs(L, True), offsets=second)
    _exact('first trip of the single launch', job, offsets=range(25))


def test_shared_launch_loops_over_items(dev, L):
    """a job of 27 x 19 = 513 work items on its 512 workgroups: item 512, the one-step last item of offset 26, is reached
    by the second trip of the job's workgroup 0.  The job is the second of the launch: its workgroups start at 2."""
    c = R.LOOP_SHARED
    small = Job(L, dev, R.SHARED_JOBS[1]['num'], R.SHARED_JOBS[1]['cap'], 32, 64, seed=12)
    job = Job(L, dev, c['num'], c['cap'], c['cin'], c['cout'], seed=13)
    jobs = [small, job]

    def run():
        assert _shared_launch(L, jobs) == 0, L.lib.ococc_last_error()
        assert _joint_reduce(L, jobs) == 0, L.lib.ococc_last_error()
    assert sorted(c['second']) == [26]
    _twice('second trip of the shared launch (offset 26)', [job], run, offsets=[26])
    _exact('first trip of the shared launch', job, offsets=range(26))
    _exact('the job in front', small)


# ---- (e) the shared launch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', R.SHARED_ORDERS, ids=lambda o: '-'.join(str(s) for s in o))
def test_shared_launch_vs_float64(dev, L, order):
    """two and three jobs per launch in both orders (shape codes 0 = 16 x 32, 1 = 32 x 64, 2 = 64 x 128; 2 selects
    wgrad_pair_kernel<true>), the jobs of one launch differing in kvol and cap; then the joint reduction of the same jobs"""
    jobs = [Job(L, dev, R.SHARED_JOBS[i]['num'], R.SHARED_JOBS[i]['cap'], *R.SHARED_SHAPES[s], seed=20 + 3 * i + s)
            for i, s in enumerate(order)]

    def run():
        assert _shared_launch(L, jobs) == 0, L.lib.ococc_last_error()
        assert _joint_reduce(L, jobs) == 0, L.lib.ococc_last_error()
    _twice(f'shared launch of shapes {order}', jobs, run)


def test_shared_launch_refusals(dev, L):
    """one job, four jobs and a 32 x 32 job: the error code, and nothing launched (the workspaces keep their NaN)"""
    jobs = [Job(L, dev, [33, 0, 513], 520, *R.SHARED_SHAPES[i % 3], seed=40 + i) for i in range(4)]
    odd = Job(L, dev, [33, 0, 513], 520, 32, 32, seed=44)
    assert _shared_launch(L, jobs[:1]) == EINVAL
    assert _shared_launch(L, jobs) == EINVAL
    assert _shared_launch(L, [jobs[0], odd]) == EUNSUPPORTED
    assert _shared_launch(L, [odd, jobs[1]]) == EUNSUPPORTED
    torch.cuda.synchronize()
    for j in jobs + [odd]:
        assert bool(j.ws.isnan().all()), 'a refused call wrote slabs'
    assert _shared_launch(L, jobs[:2]) == 0     # (the same jobs are served once the call is well formed)
    assert _joint_reduce(L, jobs[:2]) == 0
    torch.cuda.synchronize()
    _exact('after the refusals, job 0', jobs[0])
    _exact('after the refusals, job 1', jobs[1])


# ---- (f) eight reductions in one call, and the joint launch with the LayerNorm sums ---------------------------------------
@pytest.fixture(scope='module')
def eight(dev, L):
    return [Job(L, dev, c['num'], c['cap'], c['cin'], c['cout'], seed=60 + i) for i, c in enumerate(R.EIGHT)]


def test_eight_reductions_in_one_call(dev, L, eight):
    def run():
        for j in eight:
            j.slabs(L, False)
        assert _joint_reduce(L, eight) == 0, L.lib.ococc_last_error()
    _twice('eight reductions', eight, run)
    for j in eight:
        j.dw.fill_(float('nan'))
    assert _joint_reduce(L, eight + eight[:1]) == EINVAL        # nine
    torch.cuda.synchronize()
    assert all(bool(j.dw.isnan().all()) for j in eight), 'a refused call wrote sums'


def test_joint_launch_with_layernorm_sums(dev, L, eight):
    """ococc_backward_param_reduce_multi: the same eight slab reductions plus three LayerNorm partial tables
    [rows, 2 c] (c columns of d gamma, then c of d beta), integers in -3..3: exact column sums as well"""
    g = torch.Generator().manual_seed(77)
    tables = [torch.randint(-3, 4, (rows, 2 * c), generator=g).float().to(dev) for rows, c in R.LN_TABLES]
    sums = [t.double().sum(0) for t in tables]
    dgamma = [torch.empty(c, dtype=torch.float32, device=dev) for _, c in R.LN_TABLES]
    dbeta = [torch.empty(c, dtype=torch.float32, device=dev) for _, c in R.LN_TABLES]
    k = len(tables)
    vpk, i32k = ctypes.c_void_p * k, ctypes.c_int32 * k

    def run():
        for t in dgamma + dbeta:
            t.fill_(float('nan'))
        for j in eight:
            j.slabs(L, False)
        rc = L.lib.ococc_backward_param_reduce_multi(
            *_reduce_args(eight), k, vpk(*[t.data_ptr() for t in tables]), i32k(*[r for r, _ in R.LN_TABLES]),
            i32k(*[c for _, c in R.LN_TABLES]), vpk(*[t.data_ptr() for t in dgamma]), vpk(*[t.data_ptr() for t in dbeta]),
            L.stream())
        assert rc == 0, L.lib.ococc_last_error()
    _twice('joint launch', eight, run)
    for (rows, c), s, dg, db in zip(R.LN_TABLES, sums, dgamma, dbeta):
        assert torch.equal(dg.double(), s[:c]), f'd gamma of the [{rows}, 2 x {c}] table differs from its float64 column sums'
        assert torch.equal(db.double(), s[c:]), f'd beta of the [{rows}, 2 x {c}] table differs from its float64 column sums'


# ---- (g) empty problems ------------------------------------------------------------------------------------------------
def test_empty_problems(dev, L):
    kvol, cin, cout = 27, 16, 32
    job = Job(L, dev, [5] * kvol, 8, cin, cout, seed=80)

    def call(n_in, cap, ws_bytes):
        return L.lib.ococc_sparse_conv_wgrad_bf16(job.x.data_ptr(), n_in, cin, job.dy.data_ptr(), N_ROWS, cout,
                                                  job.pairs.data_ptr(), job.num.data_ptr(), kvol, cap, job.dw.data_ptr(),
                                                  job.ws.data_ptr(), ws_bytes, L.stream())
    for what, n_in, cap in (('pair_capacity = 0', N_ROWS, 0), ('n_in = 0', 0, 8)):
        job.poison()
        need = int(L.lib.ococc_sparse_conv_wgrad_workspace_bytes(kvol, cap, cin, cout))
        assert 0 < need <= job.ws.numel() * 4
        assert call(n_in, cap, need) == 0, L.lib.ococc_last_error()
        torch.cuda.synchronize()
        assert bool((job.dw == 0).all()), f'{what}: dW is not all zero'
    job.poison()
    need = int(L.lib.ococc_sparse_conv_wgrad_workspace_bytes(kvol, 8, cin, cout))
    assert need == job.ws.numel() * 4
    assert call(N_ROWS, 8, need - 1) == EINVAL
    torch.cuda.synchronize()
    assert bool(job.dw.isnan().all()) and bool(job.ws.isnan().all()), 'a refused call wrote'
    assert call(N_ROWS, 8, need) == 0
    torch.cuda.synchronize()
    _exact('the exact workspace size', job)


# ---- (h) one numeric case ----------------------------------------------------------------------------------------------
def test_normal_values_within_the_summation_bound(dev, L):
    """the densest case (513 slabs) at 64 x 128 with normal bf16 values.  Products of two bf16 numbers are exact in float32,
    so the error is that of num[k] - 1 float32 additions in some order, each at most one ulp (2^-23 relative) of a partial
    sum that |x|^T C |dy| bounds: |dW - float64| <= num[k] * 2^-23 * (|x|^T C_k |dy|).  Derived and loose."""
    c = R.REDUCE_CASES['deep_513']
    job = Job(L, dev, c['num'], max(c['num']), *R.REDUCE_BIG, seed=90, values='normal')
    absolute = R.wgrad_f64(job.x, job.dy, job.pairs, job.num, absolute=True)
    bound = torch.tensor(c['num'], dtype=torch.float64, device=dev)[:, None, None] * 2.0 ** -23 * absolute
    worst = 0.0
    for reduce in (True, False):
        job.poison()
        job.slabs(L, reduce)
        if not reduce:
            assert _joint_reduce(L, [job]) == 0, L.lib.ococc_last_error()
        torch.cuda.synchronize()
        err = (job.dw.double() - job.ref).abs()
        assert not bool(err.isnan().any())
        ratio = float((err / bound.clamp_min(1e-300)).max())
        print(f'WGRADEDGE normal 64 x 128, {"wgrad_reduce_kernel" if reduce else "wgrad_reduce_multi_kernel"}: '
              f'worst error / bound {ratio:.3e}, worst error {float(err.max()):.3e}')
        worst = max(worst, ratio)
        assert bool((err <= bound).all()), f'error / bound {ratio}'
        assert float(job.dw[1].abs().max()) == 0, 'the empty offset'
    assert worst > 0, 'normal values are not summed exactly: a zero error means the comparison compared nothing'
