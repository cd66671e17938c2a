"""One attention step against a K/V cache past 256 frames (csrc/causal_attn_step.hip,
ococc_temporal_attention_step_long_f32): the second instance of the step kernel's template, which keeps the scores in LDS
(a thread owns the scores tid, tid + 256, ...) and can address the cache as a ring (frame f in row f % cap).

1. where both exports apply (cap <= 256, no ring) the long one gives bit for bit what ococc_temporal_attention_step_f32 gives;
2. a ring cache against the operator chain softmax(scale q K^T) V in float64 with every row outside the frames lo..t-1
   poisoned, frame counts up to 2 000 000 011, and what the call may touch: row t % cap of the stepping slots, nothing else;
3. a long cache without a window, more than 256 keys, against the same chain -- held to twice the error of the f32 operator
   chain of MultiheadAttention.forward on the same row, measured here (the project's 2e-6 was set for at most 256 keys);
4. successive steps from a NaN-filled cache against the full-sequence kernel (ring) and the float64 chain (long);
5. invalid arguments launch nothing.

The float64 chain and the poison method restate those of tests/test_gpu_attention_step.py."""
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


def _launch_long(q, k_new, v_new, slot, pos, kc, vc, H, D, window, ring, out):
    from objectcentricocccompletion_amd import _lib as L
    slots, cap = kc.shape[0], kc.shape[1]
    return L.lib.ococc_temporal_attention_step_long_f32(
        q.data_ptr(), q.stride(0), k_new.data_ptr(), k_new.stride(0), v_new.data_ptr(), v_new.stride(0), slot.data_ptr(),
        pos.data_ptr(), kc.data_ptr(), vc.data_ptr(), q.shape[0], slots, cap, H, D, float(D) ** -0.5, int(window), int(ring),
        out.data_ptr(), out.stride(0), L.stream())


def _launch_old(q, k_new, v_new, slot, pos, kc, vc, H, D, window, out):
    from objectcentricocccompletion_amd import _lib as L
    slots, cap = kc.shape[0], kc.shape[1]
    return L.lib.ococc_temporal_attention_step_f32(
        q.data_ptr(), q.stride(0), k_new.data_ptr(), k_new.stride(0), v_new.data_ptr(), v_new.stride(0), slot.data_ptr(),
        pos.data_ptr(), kc.data_ptr(), vc.data_ptr(), q.shape[0], slots, cap, H, D, float(D) ** -0.5, int(window),
        out.data_ptr(), out.stride(0), L.stream())


def _lo(t, window):
    return max(0, t - window + 1) if window > 0 else 0


def _row(f, cap, ring):
    return f % cap if ring else f


def _chain64(q, k_new, v_new, kc, vc, slot_list, pos_list, H, D, window, ring):
    """float64 on the host: per row and head softmax(q . K[frames lo..t] / sqrt(D)) V[frames lo..t], frame t the new key /
    value, frame f < t in cache row f % cap (ring) or f"""
    cap = kc.shape[1]
    out = torch.zeros(len(slot_list), H * D, dtype=torch.float64)
    for i, s in enumerate(slot_list):
        t = pos_list[s]
        rows = [_row(f, cap, ring) for f in range(_lo(t, window), t)]
        K = torch.cat([kc[s, rows].double(), k_new[i:i + 1].double()], 0).view(-1, H, D)
        V = torch.cat([vc[s, rows].double(), v_new[i:i + 1].double()], 0).view(-1, H, D)
        scores = torch.einsum('hd,shd->hs', q[i].double().view(H, D) * D ** -0.5, K)
        out[i] = torch.einsum('hs,shd->hd', torch.softmax(scores, -1), V).reshape(H * D)
    return out


def _chain32(q, k_new, v_new, kc, vc, s, t, H, D, dev):
    """the f32 operator chain of MultiheadAttention.forward (the path OCOCC_FUSED_ATTENTION=0 takes and every sequence of
    more than 256 frames takes offline) for the one query row i = 0 over the frames 0..t of slot s: scaled scores by
    gemm.bmm, torch.softmax, gemm.bmm with the values, on the device"""
    from objectcentricocccompletion_amd import gemm
    heads = lambda x, n: x.reshape(n, -1, D).transpose(0, 1)                       # MultiheadAttention._heads
    K = torch.cat([kc[s, :t], k_new[:1]], 0).to(dev)
    V = torch.cat([vc[s, :t], v_new[:1]], 0).to(dev)
    scores = gemm.bmm(heads(q[:1].to(dev) * (D ** -0.5), 1), heads(K, t + 1).transpose(1, 2))
    return gemm.bmm(torch.softmax(scores, dim=-1), heads(V, t + 1)).transpose(0, 1).reshape(1, H * D)


def _err(out, ref):
    return float((out.double().cpu() - ref).abs().max() / ref.abs().max())


def _inputs(H, D, cap, slots, slot_list, pos_list, window, ring, seed):
    """random rows; both caches hold random history at the rows of the frames lo..t-1 of the stepping slots and NaN in
    every other row -- everything the kernel has no business reading"""
    g = torch.Generator().manual_seed(seed * 7919 + H * 1000 + D + cap + sum(p % 1009 for p in pos_list) + 31 * max(window, 0))
    E, n = H * D, len(slot_list)
    q, k_new, v_new = (torch.randn(n, E, generator=g) for _ in range(3))
    kc, vc = (torch.full((slots, cap, E), float('nan')) for _ in range(2))
    for s in slot_list:
        t = pos_list[s]
        rows = [_row(f, cap, ring) for f in range(_lo(t, window), t)]
        assert len(set(rows)) == len(rows) and _row(t, cap, ring) not in rows
        for c in (kc, vc):
            c[s, rows] = torch.randn(len(rows), E, generator=g)
    return q, k_new, v_new, kc, vc


def _case(dev, H, D, cap, slots, slot_list, pos_list, window, ring, seed=0):
    """one launch of the long export; the footprint checks; returns (norm-wise error against float64, out, inputs)"""
    from objectcentricocccompletion_amd import _lib as L
    q, k_new, v_new, kc, vc = _inputs(H, D, cap, slots, slot_list, pos_list, window, ring, seed)
    ref = _chain64(q, k_new, v_new, kc, vc, slot_list, pos_list, H, D, window, ring)
    d = lambda t: t.to(dev)
    kc_d, vc_d = d(kc), d(vc)
    before = (kc_d.view(torch.int32).clone(), vc_d.view(torch.int32).clone())
    out = torch.full((len(slot_list), H * D), float('nan'), device=dev)
    q_d, k_d, v_d = d(q), d(k_new), d(v_new)
    L.check(_launch_long(q_d, k_d, v_d, d(torch.tensor(slot_list, dtype=torch.int32)), d(torch.tensor(pos_list, dtype=torch.int32)),
                         kc_d, vc_d, H, D, window, ring, out), 'temporal_attention_step_long')
    assert bool(torch.isfinite(out).all())
    # footprint: the row of frame t of each stepping slot is the new key / value bit for bit, every other word is as before
    for cache, was, new in ((kc_d, before[0], k_d), (vc_d, before[1], v_d)):
        now = cache.view(torch.int32).clone()
        for i, s in enumerate(slot_list):
            r = _row(pos_list[s], cap, ring)
            assert torch.equal(now[s, r], new[i].view(torch.int32))
            now[s, r] = was[s, r]
        assert torch.equal(now, was)
    err = _err(out, ref)
    print(f'H {H} D {D} cap {cap} ring {ring} slots {slot_list} pos {[pos_list[s] for s in slot_list]} window {window}: '
          f'{err:.3e}')
    return err, out, (q, k_new, v_new, kc, vc)


# --------------------------------------------------------------------------------------------------------------------- 1
SAME = [(4, 384, 256, p) for p in (0, 1, 16, 255)] + [(1, 8, 8, p) for p in (0, 3, 7)]


@pytest.mark.parametrize('H,D,cap,pos', SAME)
def test_long_export_equals_the_step_export_where_both_apply(dev, H, D, cap, pos):
    """one kernel template, the same order of operations for <= 256 keys: out and both caches are bit-identical"""
    g = torch.Generator().manual_seed(1000 * H + D + pos)
    E = H * D
    for window in (0, 1, 3):
        q, k_new, v_new = (torch.randn(1, E, generator=g).to(dev) for _ in range(3))
        kc, vc = (torch.randn(2, cap, E, generator=g).to(dev) for _ in range(2))
        slot = torch.tensor([1], dtype=torch.int32, device=dev)
        p = torch.tensor([3, pos], dtype=torch.int32, device=dev)
        got = []
        for which in ('old', 'long'):
            k_c, v_c, out = kc.clone(), vc.clone(), torch.full((1, E), float('nan'), device=dev)
            rc = _launch_old(q, k_new, v_new, slot, p, k_c, v_c, H, D, window, out) if which == 'old' else \
                _launch_long(q, k_new, v_new, slot, p, k_c, v_c, H, D, window, 0, out)
            assert rc == 0
            got.append((out, k_c, v_c))
        dist = float((got[0][0].double() - got[1][0].double()).abs().max() / got[0][0].double().abs().max())
        print(f'H {H} D {D} cap {cap} pos {pos} window {window}: long against step export {dist:.3e}')
        assert bool(torch.isfinite(got[0][0]).all())
        for a, b in zip(*got):
            assert torch.equal(a, b), (window, dist)
        assert torch.equal(got[1][1][1, pos], k_new[0]) and torch.equal(got[1][2][1, pos], v_new[0])


# --------------------------------------------------------------------------------------------------------------------- 2
def _ring_frames(cap, window):
    return [cap - 1, cap, cap + 1, 2 * cap, 2 * cap + window - 1, 1000, 2_000_000_011]


@pytest.mark.parametrize('H,D', [(1, 8), (4, 384)])
@pytest.mark.parametrize('cap,window', [(1, 1), (3, 3), (5, 3), (16, 16), (17, 16)])
def test_ring_vs_float64_chain_and_footprint(dev, H, D, cap, window):
    """every frame count of the list, three rows at different frame counts in the non-adjacent slots 4, 0, 2 of a
    five-slot cache per launch.  Each slot's history sits at the rows f % cap of the frames lo..t-1; every other row --
    the one frame t is written to among them -- and every row of the slots 1 and 3 is NaN before the launch.  The output is
    finite and within the bound (at most 16 keys: fewer than the cases the 2e-6 already covers), row t % cap is the new key /
    value bit for bit, every other word of both caches is bit-identical."""
    ts = _ring_frames(cap, window)
    for a, b, c in ((0, 1, 2), (3, 4, 5), (6, 0, 3)):
        pos = [ts[b], 5, ts[c], 7, ts[a]]                                    # slots 4, 0, 2 step; 1 and 3 do not
        err, _, _ = _case(dev, H, D, cap, 5, [4, 0, 2], pos, window, ring=1)
        assert err <= BOUND, (pos, err)


def test_ring_window_of_one_returns_the_new_value(dev):
    """window 1: the softmax of one element is 1, the output IS the new value, at any frame count"""
    for cap in (1, 3):
        _, out, (_, _, v_new, _, _) = _case(dev, 4, 384, cap, 2, [1], [0, 2_000_000_011], 1, ring=1)
        assert torch.equal(out.cpu(), v_new)


# --------------------------------------------------------------------------------------------------------------------- 3
LONG = [(1, 8, 257, t) for t in (255, 256)] + [(1, 8, 600, t) for t in (255, 256, 257, 511, 512, 599)] + [(4, 384, 300, 299)]


def _long_bound(e_chain):
    """the project's 2e-6 was set for at most 256 keys; past that the yardstick is existing code on the same row, with the
    factor 2 DESIGN 3.14 allows for f32 arithmetic at another shape"""
    return max(BOUND, 2 * e_chain)


@pytest.mark.parametrize('H,D,cap,t', LONG)
def test_long_cache_vs_float64_chain(dev, H, D, cap, t):
    """no window, up to 600 keys: several scores per thread.  Rows t.. of the stepping slot and the whole other slot are NaN."""
    err, _, (q, k_new, v_new, kc, vc) = _case(dev, H, D, cap, 2, [1], [3, t], 0, ring=0)
    ref = _chain64(q, k_new, v_new, kc, vc, [1], [3, t], H, D, 0, 0)
    e_chain = _err(_chain32(q, k_new, v_new, kc, vc, 1, t, H, D, dev), ref)
    print(f'H {H} D {D} cap {cap} t {t}: kernel {err:.3e}, f32 operator chain {e_chain:.3e}, bound {_long_bound(e_chain):.3e}')
    assert err <= _long_bound(e_chain), (err, e_chain)


# --------------------------------------------------------------------------------------------------------------------- 4
def _future_mask(L, window, dev):
    """OccBBoxHead.get_future_mask: True = may not attend"""
    mask = torch.triu(torch.ones(L, L, dtype=torch.bool, device=dev), diagonal=1)
    if window > 0:
        for i in range(window - 1, L):
            mask[i, :i - window + 1] = True
    return mask


def _steps(dev, q, k, v, B, H, D, Lq, cap, window, ring):
    """Lq steps of B tracklets from NaN-filled caches, pos bumped by the caller after each; rows l * B + b like the input"""
    from objectcentricocccompletion_amd import _lib as L
    E = H * D
    kc, vc = (torch.full((B, cap, E), float('nan'), device=dev) for _ in range(2))
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    slot = torch.arange(B - 1, -1, -1, dtype=torch.int32, device=dev)            # row i of a step is tracklet slot[i]
    rows = []
    for l in range(Lq):
        take = l * B + slot.long()
        out = torch.empty(B, E, device=dev)
        L.check(_launch_long(q[take].contiguous(), k[take].contiguous(), v[take].contiguous(), slot, pos, kc, vc, H, D, window,
                             ring, out), 'temporal_attention_step_long')
        pos += 1
        rows.append(out[slot.long().argsort()])
    return torch.stack(rows, 0).view(Lq * B, E), kc


def test_successive_ring_steps_reproduce_the_full_kernel(dev):
    """40 steps through a ring of cap = window = 5 rows, every row overwritten eight times, against the rows of
    ococc_temporal_attention_fwd_f32 over L = 40 under the windowed future mask: within 4e-6, the sum of the two kernels'
    2e-6 bounds against float64, as tests/test_gpu_attention_step.py holds the step kernel"""
    from objectcentricocccompletion_amd.occ.layers import _TemporalAttention
    B, H, D, Lq, W = 2, 4, 384, 40, 5
    E = H * D
    g = torch.Generator().manual_seed(12)
    q, k, v = (torch.randn(Lq * B, E, generator=g).to(dev) for _ in range(3))     # token-major rows l * B + b
    mask = _future_mask(Lq, W, dev)
    full = _TemporalAttention.apply(q, k, v, mask.view(torch.uint8), None, (B, H, Lq, Lq, D), 0.0, None)
    steps, kc = _steps(dev, q, k, v, B, H, D, Lq, W, W, 1)
    assert bool(torch.isfinite(steps).all())
    err = float((steps.double() - full.double()).abs().max() / full.double().abs().max())
    print(f'40 ring steps against the full kernel: {err:.3e}')
    assert err <= 4e-6, err
    last = k.view(Lq, B, E)[Lq - W:]                                              # frames 35..39 sit in rows 0..4
    assert torch.equal(kc.transpose(0, 1), last)


def test_successive_long_steps_reproduce_the_float64_chain(dev):
    """300 steps through a long cache of 300 rows at (B, H, D) = (1, 1, 8) against the float64 chain under the plain
    future mask; the yardstick is the f32 operator chain of MultiheadAttention.forward over the same 300 frames"""
    from objectcentricocccompletion_amd import gemm
    B, H, D, Lq = 1, 1, 8, 300
    g = torch.Generator().manual_seed(13)
    q, k, v = (torch.randn(Lq, D, generator=g) for _ in range(3))
    mask = _future_mask(Lq, -1, 'cpu')
    scores = (q.double() * D ** -0.5) @ k.double().t()
    ref = torch.softmax(scores.masked_fill(mask, float('-inf')), -1) @ v.double()
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    s32 = gemm.bmm((qd * (D ** -0.5))[None], kd.t()[None]).masked_fill(mask.to(dev)[None], float('-inf'))
    e_chain = _err(gemm.bmm(torch.softmax(s32, dim=-1), vd[None])[0], ref)
    steps, kc = _steps(dev, qd, kd, vd, B, H, D, Lq, Lq, 0, 0)
    assert bool(torch.isfinite(steps).all())
    err = _err(steps, ref)
    print(f'300 long steps: kernel {err:.3e}, f32 operator chain {e_chain:.3e}, bound {_long_bound(e_chain):.3e}')
    assert err <= _long_bound(e_chain), (err, e_chain)
    assert torch.equal(kc[0], kd)                                                 # the cache holds the keys, in order


# --------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize('cap,D,window,ring,n', [(4097, 8, 0, 0, 1), (8, 6, 0, 0, 1), (8, 8, 0, 1, 1), (8, 8, -1, 1, 1),
                                                 (8, 8, 9, 1, 1), (4097, 8, 3, 1, 1), (8, 8, 0, 0, 2)])
def test_invalid_arguments_launch_nothing(dev, cap, D, window, ring, n):
    from objectcentricocccompletion_amd import _lib as L
    H, E = 2, 2 * D
    q = torch.randn(n, 16, device=dev)
    kc, vc = torch.randn(1, cap, E, device=dev), torch.randn(1, cap, E, device=dev)
    out = torch.full((n, 16), 7.0, device=dev)
    keep = (kc.clone(), vc.clone(), out.clone())
    zero = torch.zeros(n, dtype=torch.int32, device=dev)
    rc = _launch_long(q, q, q, zero, zero[:1], kc, vc, H, D, window, ring, out)
    assert rc != 0
    with pytest.raises(L.OcoccError):
        L.check(rc, 'temporal_attention_step_long')
    torch.cuda.synchronize()
    assert torch.equal(kc, keep[0]) and torch.equal(vc, keep[1]) and torch.equal(out, keep[2])
