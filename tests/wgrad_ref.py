"""Plain float64 reference of the sparse convolution's weight gradient, dW[k] = sum over the pairs of offset k of
x[in]^T dy[out], with pair lists written by hand, and a Python restatement of how csrc/sparse_conv.hip cuts that sum into
work items, slabs and reduction units.  No project imports: tests/test_gpu_wgrad_edges.py compares the HIP kernels with
this file, tests/test_wgrad_ref_cpu.py checks this file against the CPU oracle and the case table against the formulas.

Why the comparison can be exact: with x and dy drawn as integers in -3..3 (exact in bf16) every product is an integer of
magnitude <= 9, and a float32 sum of them is exact while it stays below 2^24 -- in the MFMA accumulators, in the slabs
and in both reductions, in any order.  So dW[k] must equal the float64 contraction bit for bit as long as
9 * num[k] < 2^24 (EXACT_LIMIT; a property of the inputs, asserted for every case on the CPU)."""
import torch

# ---- the partition constants of csrc/sparse_conv.hip (test_wgrad_ref_cpu.py reads them from the source and compares) ----
K_WG_STEPS = 16        # kWgSteps: 32-pair steps per work item; one work item writes one slab
K_WG_GRID = 2048       # kWgGrid: workgroups of the single launch; a job of the shared launch gets a quarter of it
K_WG_DEPTH = 4         # kWgDepth: steps whose rows are in flight in registers
K_REDUCE_GRID = 2048   # kReduceGrid: workgroups of the joint reductions
WIDE_SLABS = 16        # an offset with at most this many slabs is summed "wide" (256 elements, one thread each)
MAX_REDUCE = 8         # kMaxReduce
EXACT_LIMIT = 2 ** 24


def steps(n):
    return (n + 31) // 32


def items(n):
    """wg_items: work items (= slabs) of an offset with n pairs"""
    return (steps(n) + K_WG_STEPS - 1) // K_WG_STEPS


def last_item_steps(n):
    """steps of the last work item of an offset with n > 0 pairs"""
    return steps(n) - (items(n) - 1) * K_WG_STEPS


def slabs_before(num, k):
    """wg_span: the first slab of offset k"""
    return sum(items(int(n)) for n in list(num)[:k])


def total_items(num):
    return slabs_before(num, len(num))


def max_groups(kvol, cap):
    """wgrad_max_groups: the slabs the workspace holds, an upper bound of total_items"""
    return (kvol * ((cap + 31) // 32) + K_WG_STEPS - 1) // K_WG_STEPS + kvol


def single_grid(kvol, cap):
    return min(max_groups(kvol, cap), K_WG_GRID)


def shared_grid(kvol, cap):
    """workgroups of one job of ococc_sparse_conv_wgrad_multi_bf16"""
    return min(max_groups(kvol, cap), K_WG_GRID // 4)


def workspace_bytes(kvol, cap, cin, cout):
    return max_groups(kvol, cap) * cin * cout * 4


def reduce_units(num, elems):
    """wgrad_reduce_multi_body: per offset ('deep' | 'wide', units).  Up to 64 offsets: an offset with more than 16
    slabs is cut into deep units of 16 elements, every other one (empty ones included) into wide units of 256; above
    64 offsets every offset is deep."""
    deep, wide = (elems + 15) // 16, (elems + 255) // 256
    if len(num) > 64:
        return [('deep', deep) for _ in num]
    return [('deep', deep) if items(int(n)) > WIDE_SLABS else ('wide', wide) for n in num]


def first_chunk(num):
    """the 64-offset chunk of wg_locate in which the first work item lies (None: no items)"""
    for k, n in enumerate(num):
        if int(n) > 0:
            return k // 64
    return None


def second_trip(num, grid):
    """{offset: [parts]} of the work items a grid of `grid` workgroups reaches only on its second trip"""
    out, g = {}, 0
    for k, n in enumerate(num):
        for part in range(items(int(n))):
            if g >= grid:
                out.setdefault(k, []).append(part)
            g += 1
    return out


# ---- inputs and the reference ---------------------------------------------------------------------------------------
def make_case(num, cap, n_in, n_out, cin, cout, seed, values='int'):
    """-> x [n_in, cin], dy [n_out, cout] (bf16), pairs [kvol, 2, cap], num [kvol] (int32), on the CPU.
    Row indices are random with repeats, the two rows of a pair differ.  The tails pairs[k, :, num[k]:cap] hold valid row
    indices that are not part of the list: a kernel that reads past num[k] gets a wrong sum, not a fault."""
    num = [int(v) for v in num]
    assert all(0 <= v <= cap for v in num) and n_in >= 2 and n_out >= 2
    g = torch.Generator().manual_seed(seed)
    if values == 'int':
        x = torch.randint(-3, 4, (n_in, cin), generator=g).to(torch.bfloat16)
        dy = torch.randint(-3, 4, (n_out, cout), generator=g).to(torch.bfloat16)
    else:
        assert values == 'normal'
        x = torch.randn(n_in, cin, generator=g).to(torch.bfloat16)
        dy = torch.randn(n_out, cout, generator=g).to(torch.bfloat16)
    kvol = len(num)
    pin = torch.randint(0, n_in, (kvol, cap), generator=g, dtype=torch.int32)
    pout = torch.randint(0, n_out, (kvol, cap), generator=g, dtype=torch.int32)
    pout = torch.where(pout == pin, (pout + 1) % n_out, pout)
    pairs = torch.stack([pin, pout], 1).contiguous()
    return x, dy, pairs, torch.tensor(num, dtype=torch.int32)


def wgrad_f64(x, dy, pairs, num, absolute=False):
    """-> [kvol, cin, cout] float64 on the device of x.  absolute: the contraction of |x| and |dy| (what a bound on the
    summation error scales with)."""
    xd, dyd = x.double(), dy.double()
    if absolute:
        xd, dyd = xd.abs(), dyd.abs()
    out = torch.zeros(pairs.shape[0], x.shape[1], dy.shape[1], dtype=torch.float64, device=x.device)
    for k, n in enumerate(num.tolist()):
        if n:
            out[k] = xd[pairs[k, 0, :n].long()].t() @ dyd[pairs[k, 1, :n].long()]
    return out


# ---- the case table --------------------------------------------------------------------------------------------------
# (a) one offset per count, kvol = 27; value = (32-pair steps, work items, steps of the last item)
STEP_COUNTS = {
    0: (0, 0, 0),          # no item at all
    1: (1, 1, 1),          # one pair: 31 padded rows of the step
    31: (1, 1, 1), 32: (1, 1, 1), 33: (2, 1, 2),        # around one step
    96: (3, 1, 3), 128: (4, 1, 4), 129: (5, 1, 5), 160: (5, 1, 5),   # 3, 4, 5 steps around the register ring of kWgDepth = 4
    511: (16, 1, 16), 512: (16, 1, 16),                 # one full item
    513: (17, 2, 1), 544: (17, 2, 1), 545: (18, 2, 2),  # two items: a last item of one step and of two
    1024: (32, 2, 16), 1025: (33, 3, 1),                # two full items, and a third
}
# the counts above in an order that is not monotone, then eleven more so that all 27 offsets differ in what follows them
STEP_NUM = [513, 0, 1, 1025, 31, 32, 33, 545, 96, 128, 129, 160, 511, 512, 544, 1024,
            2, 64, 65, 127, 480, 1023, 1056, 1057, 1536, 1537, 0]
STEP_CAP = 1600            # above every count: each list has a tail
CHANNELS = (16, 32, 64, 128)

# (b) kvol = 4, slabs per offset around the wide/deep rule (16 / 17), the u + 8 half of the wide sum (8 / 9) and the
# 16-way unrolled loop of the deep sum (lane p takes slabs p, p + 16, ..., the loop runs while p + 240 < slabs: 240 / 241
# is its first trip for lane 0, 256 / 257 one trip of every lane and the first slab behind it, 513 two trips and a slab).
# slabs: what items() must give; deep: which offsets the joint reduction sums deep
REDUCE_CASES = {
    'wide_8_9_16_17': dict(num=[4096, 4097, 8192, 8193], slabs=[8, 9, 16, 17], deep=[False, False, False, True],
                           why='8|9 slabs: the u + 8 half; 16|17: wide|deep, a deep offset behind three wide ones'),
    'deep_after_empty': dict(num=[0, 122880, 122881, 512], slabs=[0, 240, 241, 1], deep=[False, True, True, False],
                             why='240|241 slabs: the unrolled deep loop not entered | entered by lane 0; deep after an empty offset'),
    'deep_after_one_slab': dict(num=[512, 131072, 131073, 4097], slabs=[1, 256, 257, 9], deep=[False, True, True, False],
                                why='256|257 slabs: one full unrolled trip | and one slab behind it; deep after a one-slab offset'),
    'deep_513': dict(num=[262656, 0, 8192, 1], slabs=[513, 0, 16, 1], deep=[True, False, False, False],
                     why='513 slabs: two unrolled trips and a remainder; the densest case (9 * 262 656 = 2.4 M < 2^24)'),
    # the 16|17 and 256|257 entries again at 64 x 128 (REDUCE_BIG): 512 deep units per offset
    'big_16_17_256_257': dict(num=[8192, 8193, 131072, 131073], slabs=[16, 17, 256, 257], deep=[False, True, True, True],
                              why='16|17 and 256|257 at 64 x 128 channels'),
}
REDUCE_SMALL, REDUCE_BIG = (16, 32), (64, 128)

# (c) offsets beyond one wave: kvol <= 64 takes the scan branch of the joint reduction, kvol > 64 the division branch
WAVE_KVOLS = (1, 63, 64, 65, 125, 129)
WAVE_CAP = 1100


def wave_num(kvol, pattern):
    """'late': the first 64 offsets are empty (kvol > 64: the first item lies in the second chunk of wg_locate; up to 64
    offsets: only the last offset has pairs).  'marks': pairs at offsets 0, 63, 64 and kvol - 1, where they exist."""
    num = [0] * kvol
    if pattern == 'late':
        if kvol > 64:
            for k in range(64, kvol):
                num[k] = (545, 33, 0, 513, 1)[(k - 64) % 5]
        num[kvol - 1] = 1025
    else:
        assert pattern == 'marks'
        for k, n in ((0, 33), (63, 513), (64, 545), (kvol - 1, 1025)):
            if k < kvol:
                num[k] = n
    return num


WAVE_CASES = {(kvol, p): dict(num=wave_num(kvol, p), chunk=1 if (p == 'late' and kvol > 64) else 0)
              for kvol in WAVE_KVOLS for p in ('late', 'marks')}

# (d) a work list longer than the grid: the items of the second trip are the ones under test
LOOP_SINGLE = dict(kvol=27, cap=40000, num=[40000] * 27, cin=16, cout=16, items_per_offset=79, items=2133, grid=2048,
                   second={25: list(range(73, 79)), 26: list(range(79))},
                   why='27 x 79 = 2 133 items on 2 048 workgroups: workgroups 0..84 take items 2 048..2 132, the last six '
                       'of offset 25 and all of offset 26')
LOOP_SHARED = dict(kvol=27, cap=9217, num=[9217] * 27, cin=16, cout=32, items_per_offset=19, items=513, grid=512,
                   second={26: [18]},
                   why='27 x 19 = 513 items on the 512 workgroups of a job: workgroup 0 of the job takes item 512, the last '
                       'item (one step, one pair) of offset 26')

# (e) jobs of the shared launch, dealt to the positions of a call in this order: different kvol and cap, a job whose
# items are all in its last offset, a job whose second item lies behind 64 offsets
SHARED_JOBS = [
    dict(num=STEP_NUM, cap=STEP_CAP),
    dict(num=[0] * 7 + [700], cap=700),
    dict(num=[33] + [0] * 63 + [1025], cap=1056),
]
SHARED_SHAPES = ((16, 32), (32, 64), (64, 128))      # shape codes 0, 1, 2 of the launch; 2 selects the BIG instantiation
SHARED_ORDERS = ((0, 1), (1, 0), (1, 2), (2, 1, 0), (0, 1, 2))

# (f) eight reductions in one call: mixed shapes, kvol 27 and 125, deep and wide
EIGHT = [
    dict(cin=16, cout=32, num=STEP_NUM, cap=STEP_CAP),
    dict(cin=32, cout=64, num=wave_num(125, 'late'), cap=WAVE_CAP),
    dict(cin=16, cout=16, num=[512, 8193, 0, 33] + [0] * 22 + [4097], cap=8200),           # deep behind a one-slab offset
    dict(cin=64, cout=128, num=STEP_NUM[::-1], cap=STEP_CAP),
    dict(cin=128, cout=16, num=wave_num(125, 'marks'), cap=WAVE_CAP),
    dict(cin=32, cout=32, num=[0, 8704, 1] + [0] * 23 + [8192], cap=8704),                  # deep behind an empty offset
    dict(cin=16, cout=64, num=[4096, 0, 8193, 512], cap=8200),
    dict(cin=64, cout=32, num=[1] * 27, cap=64),
]
LN_TABLES = [(1, 16), (37, 64), (1100, 100)]      # (partial rows, c): one row, a few, and more than 32 lanes x 32 sums


CASES = dict(steps=dict(num=STEP_NUM, cap=STEP_CAP, counts=STEP_COUNTS), reduce=REDUCE_CASES, wave=WAVE_CASES,
             loop_single=LOOP_SINGLE, loop_shared=LOOP_SHARED, shared_jobs=SHARED_JOBS, eight=EIGHT, ln_tables=LN_TABLES)


def all_nums():
    """(name, num) of every case of the table"""
    yield 'steps', STEP_NUM
    for name, c in REDUCE_CASES.items():
        yield name, c['num']
    for key, c in WAVE_CASES.items():
        yield 'wave%s' % (key,), c['num']
    yield 'loop_single', LOOP_SINGLE['num']
    yield 'loop_shared', LOOP_SHARED['num']
    for i, c in enumerate(SHARED_JOBS):
        yield 'shared_job%d' % i, c['num']
    for i, c in enumerate(EIGHT):
        yield 'eight%d' % i, c['num']
