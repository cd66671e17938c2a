"""Several frames per slot in one attention call (csrc/causal_attn_step.hip, ococc_temporal_attention_chunk_f32): the
chunk mode of the step kernel's template.  Row i is frame pos[slot] + off[i] of its slot; it takes the keys and values of the
frames before pos[slot] from the cache and those of the call's own frames from k_new / v_new, and a second kernel of the same
call appends the new rows afterwards.

1. bit identity with the corresponding sequence of ococc_temporal_attention_step_f32 / _step_long_f32 calls (pos bumped in
   between): out and both caches;
2. against the operator chain softmax(scale q K^T) V in float64 with NaN in every cache row no row of the call may read
   (without ring that includes the rows the new frames go to), and what the call may touch: the rows of the new frames;
3. a whole sequence as ONE chunk from a NaN-filled cache against ococc_temporal_attention_fwd_f32 under the future mask;
4. rows the device-side guards refuse are skipped; invalid arguments launch nothing.

The float64 chain, the poison method and the bounds restate those of tests/test_gpu_attention_step_long.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 2e-6   # norm-wise against float64: the project's bound for attention over at most 256 keys


@pytest.fixture(scope='module', autouse=True)
def _generators_as_found():
    """later tests of the suite initialise networks from torch's global generators without seeding them: leave both
    as this module found them"""
    cpu = torch.get_rng_state()
    gpu = torch.cuda.get_rng_state() if torch.cuda.is_available() else None
    yield
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state(gpu)


def _launch_chunk(q, k_new, v_new, slot, off, pos, kc, vc, H, D, window, ring, out):
    from objectcentricocccompletion_amd import _lib as L
    slots, cap = kc.shape[0], kc.shape[1]
    return L.lib.ococc_temporal_attention_chunk_f32(
        q.data_ptr(), q.stride(0), k_new.data_ptr(), k_new.stride(0), v_new.data_ptr(), v_new.stride(0), slot.data_ptr(),
        off.data_ptr(), pos.data_ptr(), kc.data_ptr(), vc.data_ptr(), q.shape[0], slots, cap, H, D, float(D) ** -0.5,
        int(window), int(ring), out.data_ptr(), out.stride(0), L.stream())


def _launch_step(q, k_new, v_new, slot, pos, kc, vc, H, D, window, ring, out):
    """one single-frame step: the first export where it applies (cap <= 256, no ring), the long one otherwise"""
    from objectcentricocccompletion_amd import _lib as L
    slots, cap = kc.shape[0], kc.shape[1]
    head = (q.data_ptr(), q.stride(0), k_new.data_ptr(), k_new.stride(0), v_new.data_ptr(), v_new.stride(0), slot.data_ptr(),
            pos.data_ptr(), kc.data_ptr(), vc.data_ptr(), q.shape[0], slots, cap, H, D, float(D) ** -0.5, int(window))
    tail = (out.data_ptr(), out.stride(0), L.stream())
    if cap <= 256 and not ring:
        return L.lib.ococc_temporal_attention_step_f32(*head, *tail)
    return L.lib.ococc_temporal_attention_step_long_f32(*head, int(ring), *tail)


def _lo(t, window):
    return max(0, t - window + 1) if window > 0 else 0


def _row(f, cap, ring):
    return f % cap if ring else f


def _offsets(slot_rows):
    """the place of each row in its slot's run (the rows of a slot are consecutive)"""
    off = []
    for i, s in enumerate(slot_rows):
        off.append(off[-1] + 1 if i and slot_rows[i - 1] == s else 0)
    return off


def _dev_i32(values, dev):
    return torch.tensor(values, dtype=torch.int32).to(dev)


def _inputs(H, D, cap, slots, slot_rows, pos_list, window, ring, seed, poison):
    """random rows.  ``poison``: both caches hold random history at the rows of the frames lo(pos)..pos-1 of the slots of
    the call -- all that any of its rows may read from the cache -- and NaN in every other row; otherwise random everywhere"""
    g = torch.Generator().manual_seed(seed * 7919 + H * 1000 + D + cap + sum(p % 1009 for p in pos_list) + 31 * max(window, 0)
                                      + 17 * len(slot_rows))
    E, n = H * D, len(slot_rows)
    q, k_new, v_new = (torch.randn(n, E, generator=g) for _ in range(3))
    if not poison:
        kc, vc = (torch.randn(slots, cap, E, generator=g) for _ in range(2))
        return q, k_new, v_new, kc, vc
    kc, vc = (torch.full((slots, cap, E), float('nan')) for _ in range(2))
    for s in dict.fromkeys(slot_rows):
        p = pos_list[s]
        rows = [_row(f, cap, ring) for f in range(_lo(p, window), p)]
        assert len(set(rows)) == len(rows)
        for c in (kc, vc):
            c[s, rows] = torch.randn(len(rows), E, generator=g)
    return q, k_new, v_new, kc, vc


def _keys(i, s, first, p, t, k_new, kc, window, ring):
    """the keys (or values) of the frames lo..t of row i: the cached frames below p, then the call's own rows"""
    cap, lo = kc.shape[1], _lo(t, window)
    cached = [_row(f, cap, ring) for f in range(lo, min(p, t + 1))]
    own = list(range(first + max(lo, p) - p, i + 1))
    return torch.cat([kc[s, cached], k_new[own]], 0)


def _chain64(q, k_new, v_new, kc, vc, slot_rows, pos_list, H, D, window, ring):
    """float64 on the host: per row and head softmax(q . K[frames lo..t] / sqrt(D)) V[frames lo..t]"""
    out = torch.zeros(len(slot_rows), H * D, dtype=torch.float64)
    for i, (s, o) in enumerate(zip(slot_rows, _offsets(slot_rows))):
        p = pos_list[s]
        K = _keys(i, s, i - o, p, p + o, k_new, kc, window, ring).double().view(-1, H, D)
        V = _keys(i, s, i - o, p, p + o, v_new, vc, window, ring).double().view(-1, H, D)
        assert K.shape[0] == p + o - _lo(p + o, window) + 1
        scores = torch.einsum('hd,shd->hs', q[i].double().view(H, D) * D ** -0.5, K)
        out[i] = torch.einsum('hs,shd->hd', torch.softmax(scores, -1), V).reshape(H * D)
    return out


def _chain32_row(q, K, V, H, D, dev):
    """the f32 operator chain of MultiheadAttention.forward (scaled scores by gemm.bmm, torch.softmax, gemm.bmm with the
    values, on the device) for one query row over the keys K / values V"""
    from objectcentricocccompletion_amd import gemm
    heads = lambda x, n: x.reshape(n, -1, D).transpose(0, 1)                       # MultiheadAttention._heads
    S = K.shape[0]
    scores = gemm.bmm(heads(q[None].to(dev) * (D ** -0.5), 1), heads(K.to(dev), S).transpose(1, 2))
    return gemm.bmm(torch.softmax(scores, dim=-1), heads(V.to(dev), S)).transpose(0, 1).reshape(H * D)


def _err(out, ref):
    return float((out.double().cpu() - ref).abs().max() / ref.abs().max())


def _long_bound(e_chain):
    """the project's 2e-6 was set for at most 256 keys; past that the yardstick is existing code on the same row, with the
    factor 2 DESIGN 3.14 allows for f32 arithmetic at another shape"""
    return max(BOUND, 2 * e_chain)


def _expected_caches(kc, vc, k_new, v_new, slot_rows, pos_list, ring):
    """the caches after the frames of the call were written in order"""
    kc, vc, cap = kc.clone(), vc.clone(), kc.shape[1]
    for i, (s, o) in enumerate(zip(slot_rows, _offsets(slot_rows))):
        r = _row(pos_list[s] + o, cap, ring)
        kc[s, r], vc[s, r] = k_new[i], v_new[i]
    return kc, vc


def _bits(t):
    return t.contiguous().view(torch.int32)


def _chunk(dev, H, D, slot_rows, pos_list, window, ring, inputs):
    """one chunk call on copies of the caches; returns out and both caches on the device"""
    from objectcentricocccompletion_amd import _lib as L
    q, k_new, v_new, kc, vc = (t.to(dev) for t in inputs)
    pos = _dev_i32(pos_list, dev)
    out = torch.full((len(slot_rows), H * D), float('nan'), device=dev)
    L.check(_launch_chunk(q, k_new, v_new, _dev_i32(slot_rows, dev), _dev_i32(_offsets(slot_rows), dev), pos, kc, vc, H, D,
                          window, ring, out), 'temporal_attention_chunk')
    assert pos.tolist() == list(pos_list)                                          # pos is left alone
    return out, kc, vc


def _singles(dev, H, D, slot_rows, pos_list, window, ring, inputs):
    """the same rows as single steps, one row per launch in input order, pos bumped in between"""
    from objectcentricocccompletion_amd import _lib as L
    q, k_new, v_new, kc, vc = (t.to(dev) for t in inputs)
    pos = _dev_i32(pos_list, dev)
    out = torch.full((len(slot_rows), H * D), float('nan'), device=dev)
    one = torch.ones(1, dtype=torch.int32, device=dev)
    slot_dev = _dev_i32(slot_rows, dev)
    for i in range(len(slot_rows)):
        L.check(_launch_step(q[i:i + 1], k_new[i:i + 1], v_new[i:i + 1], slot_dev[i:i + 1], pos, kc, vc, H, D, window, ring,
                             out[i:i + 1]), 'temporal_attention_step')
        pos.index_add_(0, slot_dev[i:i + 1].long(), one)
    return out, kc, vc


def _assert_bit_identical(dev, H, D, cap, slots, slot_rows, pos_list, window, ring, seed=0):
    inputs = _inputs(H, D, cap, slots, slot_rows, pos_list, window, ring, seed, poison=False)
    got, want = _chunk(dev, H, D, slot_rows, pos_list, window, ring, inputs), \
        _singles(dev, H, D, slot_rows, pos_list, window, ring, inputs)
    tag = f'H {H} D {D} cap {cap} ring {ring} rows {slot_rows if len(slot_rows) <= 8 else len(slot_rows)} pos {pos_list} ' \
          f'window {window}'
    assert bool(torch.isfinite(want[0]).all()), tag
    dist = float((got[0].double() - want[0].double()).abs().max() / want[0].double().abs().max())
    print(f'{tag}: chunk against single steps {dist:.3e}')
    for name, a, b in zip(('out', 'k_cache', 'v_cache'), got, want):
        assert torch.equal(_bits(a), _bits(b)), (tag, name, dist)
    exp = _expected_caches(inputs[3], inputs[4], inputs[1], inputs[2], slot_rows, pos_list, ring)
    assert torch.equal(got[1].cpu(), exp[0]) and torch.equal(got[2].cpu(), exp[1]), tag


def _assert_close_to_float64(dev, H, D, cap, slots, slot_rows, pos_list, window, ring, seed=1):
    """NaN everywhere the call may not read; out finite and within the bound row by row; the footprint"""
    inputs = _inputs(H, D, cap, slots, slot_rows, pos_list, window, ring, seed, poison=True)
    q, k_new, v_new, kc, vc = inputs
    ref = _chain64(q, k_new, v_new, kc, vc, slot_rows, pos_list, H, D, window, ring)
    out, kc_d, vc_d = _chunk(dev, H, D, slot_rows, pos_list, window, ring, inputs)
    assert bool(torch.isfinite(out).all())
    worst = 0.0
    for i, (s, o) in enumerate(zip(slot_rows, _offsets(slot_rows))):
        p = pos_list[s]
        t = p + o
        nk = t - _lo(t, window) + 1
        err, bound = _err(out[i], ref[i]), BOUND
        if nk > 256:
            K, V = (_keys(i, s, i - o, p, t, new, c, window, ring) for new, c in ((k_new, kc), (v_new, vc)))
            e_chain = _err(_chain32_row(q[i], K, V, H, D, dev), ref[i])
            bound = _long_bound(e_chain)
            print(f'row {i}: {nk} keys, kernel {err:.3e}, f32 operator chain {e_chain:.3e}, bound {bound:.3e}')
        worst = max(worst, err)
        assert err <= bound, (i, nk, err, bound)
    print(f'H {H} D {D} cap {cap} ring {ring} rows {slot_rows if len(slot_rows) <= 8 else len(slot_rows)} pos {pos_list} '
          f'window {window}: worst row {worst:.3e}')
    # footprint: exactly the rows of the new frames changed, bit-equal to k_new / v_new (NaN rows compare by their bits)
    exp = _expected_caches(kc, vc, k_new, v_new, slot_rows, pos_list, ring)
    assert torch.equal(_bits(kc_d.cpu()), _bits(exp[0])) and torch.equal(_bits(vc_d.cpu()), _bits(exp[1]))


# the cases of both checks: (H, D, cap, slots, slot rows, pos per slot, windows, ring)
def _plain_cases():
    cases = []
    for start in (0, 3):                                                           # short
        for run in (1, 2, 5):
            cases.append((1, 8, 8, 2, [1] * run, [2, start], (0, 1, 3)))
    for start, run in ((0, 17), (14, 4), (250, 6)):                                # 256-key: 15..18 keys cross the 16-key pass
        cases.append((4, 384, 256, 2, [1] * run, [3, start], (0,)))
    cases.append((2, 8, 12, 5, [4, 4, 4, 0, 2, 2], [7, 1, 0, 2, 5], (0, 3)))       # multi-slot, different starts
    cases.append((1, 8, 600, 2, [1] * 10, [3, 250], (0,)))                         # long: 251..260 keys
    return [(H, D, cap, slots, rows, pos, w) for H, D, cap, slots, rows, pos, ws in cases for w in ws]


PLAIN = _plain_cases()
RING = [(1, 1), (3, 3), (5, 3), (16, 16), (17, 16)]


def _ring_calls(cap):
    """(start, run) over the starts 0, cap - 1, 2 cap, 2 000 000 000 and the runs 1, cap, cap + 1, 2 cap + 1"""
    return [(start, run) for start in dict.fromkeys((0, cap - 1, 2 * cap, 2_000_000_000))
            for run in dict.fromkeys((1, cap, cap + 1, 2 * cap + 1))]


# --------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('H,D,cap,slots,slot_rows,pos_list,window', PLAIN)
def test_chunk_is_bit_identical_to_single_steps(dev, H, D, cap, slots, slot_rows, pos_list, window):
    """one kernel template, the same order of operations over the keys lo..t, whether a key comes from the cache or from
    the call's own rows: out and both caches are bit-identical to those the single steps leave"""
    _assert_bit_identical(dev, H, D, cap, slots, slot_rows, pos_list, window, 0)


@pytest.mark.parametrize('H,D', [(2, 8), (4, 384)])
@pytest.mark.parametrize('cap,window', RING)
def test_ring_chunk_is_bit_identical_to_single_steps(dev, H, D, cap, window):
    """runs up to 2 cap + 1 frames through a ring of cap rows, from frame counts up to 2 000 000 000, next to a second
    slot that takes one frame in the same call: out as the single steps give it, and the final caches hold, row by row,
    the frame the single steps leave there (a run longer than cap overwrites its own frames)"""
    for start, run in _ring_calls(cap):
        _assert_bit_identical(dev, H, D, cap, 3, [2] * run + [0], [start + 1, 9, start], window, 1)


# --------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('H,D,cap,slots,slot_rows,pos_list,window', PLAIN)
def test_chunk_vs_float64_chain_and_footprint(dev, H, D, cap, slots, slot_rows, pos_list, window):
    """every cache row the call may not read is NaN -- the rows its new frames go to among them, which catches a key of
    the chunk taken from the cache -- and every row of the slots that do not step"""
    _assert_close_to_float64(dev, H, D, cap, slots, slot_rows, pos_list, window, 0)


@pytest.mark.parametrize('cap,window', RING)
def test_ring_chunk_vs_float64_chain_and_footprint(dev, cap, window):
    """a ring holds random history at the rows f % cap of the frames lo(pos)..pos - 1 and NaN elsewhere; at most 16 keys"""
    for start, run in _ring_calls(cap):
        _assert_close_to_float64(dev, 2, 8, cap, 3, [2] * run + [0], [start + 1, 9, start], window, 1)


def test_ring_window_of_one_returns_the_new_values(dev):
    """window 1: the softmax of one element is 1, every row of the chunk IS its own value"""
    inputs = _inputs(4, 384, 3, 2, [1] * 7, [0, 2_000_000_000], 1, 1, 3, poison=True)
    out, _, _ = _chunk(dev, 4, 384, [1] * 7, [0, 2_000_000_000], 1, 1, inputs)
    assert torch.equal(out.cpu(), inputs[2])


# --------------------------------------------------------------------------------------------------------------------- 3
def _future_mask(L, window, dev):
    """OccBBoxHead.get_future_mask: True = may not attend"""
    mask = torch.triu(torch.ones(L, L, dtype=torch.bool, device=dev), diagonal=1)
    if window > 0:
        for i in range(window - 1, L):
            mask[i, :i - window + 1] = True
    return mask


@pytest.mark.parametrize('window,cap,ring', [(5, 5, 1), (-1, 40, 0)])
def test_a_whole_sequence_as_one_chunk_reproduces_the_full_kernel(dev, window, cap, ring):
    """(B, H, D, L) = (2, 4, 384, 40) from NaN-filled caches in ONE call -- through a ring of cap = window = 5 rows, every
    row of which eight frames of the call pass through, and without a window through a plain cache of 40 rows -- against
    the rows of ococc_temporal_attention_fwd_f32 under the future mask: within 4e-6, the sum of the two kernels' 2e-6
    bounds against float64, as tests/test_gpu_attention_step.py holds the step kernel"""
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ.layers import _TemporalAttention
    B, H, D, Lq = 2, 4, 384, 40
    E = H * D
    g = torch.Generator().manual_seed(12)
    q, k, v = (torch.randn(Lq * B, E, generator=g).to(dev) for _ in range(3))     # token-major rows l * B + b
    full = _TemporalAttention.apply(q, k, v, _future_mask(Lq, window, dev).view(torch.uint8), None, (B, H, Lq, Lq, D), 0.0, None)
    slot_rows = [1] * Lq + [0] * Lq                                               # tracklet 1 first: rows b, then frame
    take = torch.tensor([l * B + b for b in (1, 0) for l in range(Lq)], device=dev)
    kc, vc = (torch.full((B, cap, E), float('nan'), device=dev) for _ in range(2))
    out = torch.full((Lq * B, E), float('nan'), device=dev)
    L.check(_launch_chunk(q[take].contiguous(), k[take].contiguous(), v[take].contiguous(), _dev_i32(slot_rows, dev),
                          _dev_i32(_offsets(slot_rows), dev), torch.zeros(B, dtype=torch.int32, device=dev), kc, vc, H, D,
                          window, ring, out), 'temporal_attention_chunk')
    assert bool(torch.isfinite(out).all())
    got = torch.empty_like(out)
    got[take] = out
    err = float((got.double() - full.double()).abs().max() / full.double().abs().max())
    print(f'one chunk of {Lq} frames, window {window}, cap {cap}, ring {ring}: against the full kernel {err:.3e}')
    assert err <= 4e-6, err
    last = k.view(Lq, B, E)[Lq - cap:]                                            # frames 35..39 sit in rows 0..4; 0..39 in 0..39
    assert torch.equal(kc.transpose(0, 1), last) and torch.equal(vc.transpose(0, 1), v.view(Lq, B, E)[Lq - cap:])


# --------------------------------------------------------------------------------------------------------------------- 4
def test_rows_the_guards_refuse_are_skipped(dev):
    """a slot out of range, off < 0, off > i, a run whose first row belongs to another slot, a frame past cap: the row's
    output and both caches stay as they were (the host layers report all of these first); the valid rows next to them
    are computed and appended"""
    from objectcentricocccompletion_amd import _lib as L
    H, D, cap, slots = 2, 8, 4, 3
    E = H * D
    slot_rows = [0, 0, 7, -1, 1, 1, 2, 2, 1]
    off = [0, 1, 0, 0, -1, 6, 1, 0, 0]          # row 4: off < 0; row 5: off > i; row 6: row 5 is slot 1, not 2; row 8: t >= cap
    pos_list = [1, 4, 0]
    valid = [0, 1, 7]
    g = torch.Generator().manual_seed(4)
    q, k_new, v_new = (torch.randn(len(slot_rows), E, generator=g).to(dev) for _ in range(3))
    kc, vc = (torch.randn(slots, cap, E, generator=g).to(dev) for _ in range(2))
    before = (kc.clone(), vc.clone())
    out = torch.full((len(slot_rows), E), 7.0, device=dev)
    L.check(_launch_chunk(q, k_new, v_new, _dev_i32(slot_rows, dev), _dev_i32(off, dev), _dev_i32(pos_list, dev), kc, vc, H, D,
                          0, 0, out), 'temporal_attention_chunk')
    skipped = [i for i in range(len(slot_rows)) if i not in valid]
    assert bool((out[skipped] == 7.0).all()) and bool(torch.isfinite(out[valid]).all()) and not bool((out[valid] == 7.0).any())
    exp_k, exp_v = before[0].clone(), before[1].clone()
    for i, (s, t) in zip(valid, ((0, 1), (0, 2), (2, 0))):
        exp_k[s, t], exp_v[s, t] = k_new[i], v_new[i]
    assert torch.equal(kc, exp_k) and torch.equal(vc, exp_v)
    ref = _chain64(q[:2].cpu(), k_new[:2].cpu(), v_new[:2].cpu(), before[0].cpu(), before[1].cpu(), [0, 0], pos_list, H, D, 0, 0)
    assert _err(out[:2], ref) <= BOUND


@pytest.mark.parametrize('cap,D,window,ring', [(4097, 8, 0, 0), (8, 6, 0, 0), (8, 388, 0, 0), (8, 8, 0, 1), (8, 8, -1, 1),
                                               (8, 8, 9, 1), (4097, 8, 3, 1)])
def test_invalid_arguments_launch_nothing(dev, cap, D, window, ring):
    from objectcentricocccompletion_amd import _lib as L
    H, n = 2, 2
    E = H * D
    q = torch.randn(n, E, device=dev)
    kc, vc = torch.randn(1, cap, E, device=dev), torch.randn(1, cap, E, device=dev)
    out = torch.full((n, E), 7.0, device=dev)
    keep = (kc.clone(), vc.clone(), out.clone())
    zero = torch.zeros(n, dtype=torch.int32, device=dev)
    rc = _launch_chunk(q, q, q, zero, _dev_i32([0, 1], dev), zero[:1], kc, vc, H, D, window, ring, out)
    assert rc != 0
    with pytest.raises(L.OcoccError):
        L.check(rc, 'temporal_attention_chunk')
    torch.cuda.synchronize()
    assert torch.equal(kc, keep[0]) and torch.equal(vc, keep[1]) and torch.equal(out, keep[2])
