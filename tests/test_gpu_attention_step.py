"""One attention step against a K/V cache (csrc/causal_attn_step.hip, ococc_temporal_attention_step_f32) -- the
single-query form of the temporal transformer's attention core for tracklets that arrive frame by frame -- against the
operator chain softmax(scale q K^T) V over the cached frames lo..t written out in float64, against the full-sequence kernel
under the causal mask, and for what it may touch: it appends row pos[slot] of its own slots and reads rows lo..pos[slot]-1,
nothing else.

The kernel takes the scores 16 keys per pass of a workgroup (kSK) and deals the keys of the value product round-robin to 16
lane groups, so the frame counts 15 / 16 / 17 sit on both sides of a pass; 63 / 64 / 65 are the sides of the chunk the
full-sequence kernel stages by; 255 is the last row of the largest cache."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 2e-6   # norm-wise against float64: the bound tests/test_gpu_temporal_attention.py holds the full kernel to


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


def _launch(q, k_new, v_new, slot, pos, kc, vc, H, D, window, out):
    from objectcentricocccompletion_amd import _lib as L
    slots, cap = kc.shape[0], kc.shape[1]
    return L.lib.ococc_temporal_attention_step_f32(
        q.data_ptr(), q.stride(0), k_new.data_ptr(), k_new.stride(0), v_new.data_ptr(), v_new.stride(0), slot.data_ptr(),
        pos.data_ptr(), kc.data_ptr(), vc.data_ptr(), q.shape[0], slots, cap, H, D, float(D) ** -0.5, int(window),
        out.data_ptr(), out.stride(0), L.stream())


def _lo(t, window):
    return max(0, t - window + 1) if window > 0 else 0


def _chain64(q, k_new, v_new, kc, vc, slot_list, pos_list, H, D, window):
    """float64 on the host: per row and head softmax(q . K[lo..t] / sqrt(D)) V[lo..t], row t the new key / value"""
    out = torch.zeros(len(slot_list), H * D, dtype=torch.float64)
    for i, s in enumerate(slot_list):
        t = pos_list[s]
        lo = _lo(t, window)
        K = torch.cat([kc[s, lo:t].double(), k_new[i:i + 1].double()], 0).view(-1, H, D)
        V = torch.cat([vc[s, lo:t].double(), v_new[i:i + 1].double()], 0).view(-1, H, D)
        scores = torch.einsum('hd,shd->hs', q[i].double().view(H, D) * D ** -0.5, K)
        out[i] = torch.einsum('hs,shd->hd', torch.softmax(scores, -1), V).reshape(H * D)
    return out


def _case(dev, H, D, cap, slots, slot_list, pos_list, window, poison, seed=0):
    """one launch; returns (norm-wise error against float64, out, the inputs) after the footprint checks"""
    from objectcentricocccompletion_amd import _lib as L
    g = torch.Generator().manual_seed(seed * 7919 + H * 1000 + D + cap + sum(pos_list) + 31 * max(window, 0))
    E, n = H * D, len(slot_list)
    q, k_new, v_new = (torch.randn(n, E, generator=g) for _ in range(3))
    kc, vc = (torch.randn(slots, cap, E, generator=g) for _ in range(2))
    if poison:   # everything the kernel has no business reading
        for c in (kc, vc):
            for s in range(slots):
                if s in slot_list:
                    t = pos_list[s]
                    c[s, :_lo(t, window)] = float('nan')
                    c[s, t:] = float('nan')
                else:
                    c[s] = float('nan')
    ref = _chain64(q, k_new, v_new, kc, vc, slot_list, pos_list, H, D, window)
    d = lambda t: t.to(dev)
    kc_d, vc_d = d(kc), d(vc)
    before = (kc_d.view(torch.int32).clone(), vc_d.view(torch.int32).clone())
    out = torch.full((n, E), float('nan'), device=dev)
    q_d, k_d, v_d = d(q), d(k_new), d(v_new)
    L.check(_launch(q_d, k_d, v_d, d(torch.tensor(slot_list, dtype=torch.int32)), d(torch.tensor(pos_list, dtype=torch.int32)),
                    kc_d, vc_d, H, D, window, out), 'temporal_attention_step')
    assert bool(torch.isfinite(out).all())
    # footprint: row t of each stepping slot is the new key / value bit for bit, every other word is as before
    for cache, was, new in ((kc_d, before[0], k_d), (vc_d, before[1], v_d)):
        now = cache.view(torch.int32).clone()
        for i, s in enumerate(slot_list):
            assert torch.equal(now[s, pos_list[s]], new[i].view(torch.int32))
            now[s, pos_list[s]] = was[s, pos_list[s]]
        assert torch.equal(now, was)
    err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f'H {H} D {D} cap {cap} slots {slot_list} pos {[pos_list[s] for s in slot_list]} window {window}: {err:.3e}')
    return err, out, v_d


CASES = [(4, 384, 256, p) for p in (0, 1, 14, 15, 16, 17, 63, 64, 65, 255)] + [(1, 8, 8, p) for p in (0, 1, 3, 7)]


@pytest.mark.parametrize('H,D,cap,pos', CASES)
def test_step_vs_float64_chain(dev, H, D, cap, pos):
    """every frame count at the model's shape and at fewer than one float4 group per lane, windows off / 1 / 3 / wider
    than the frames there are; at pos = 0 the softmax of one element is 1 and the output IS the new value"""
    for window in (0, 1, 3, pos + 5):
        err, out, v_new = _case(dev, H, D, cap, 2, [1], [3, pos], window, poison=False)
        assert err <= BOUND, (window, err)
        if pos == 0 or window == 1:
            assert torch.equal(out, v_new)


@pytest.mark.parametrize('H,D,cap', [(4, 384, 256), (1, 8, 8)])
@pytest.mark.parametrize('window', [0, 1, 3, 300])
def test_step_rows_in_separate_slots_and_footprint(dev, H, D, cap, window):
    """one launch, three rows at different frame counts in non-adjacent slots of a five-slot cache; every cache row outside
    [lo, t-1] of the stepping slots and every row of the other slots is NaN before the launch: the output is finite and
    within the bound, row t is the new key / value bit for bit, every other word of both caches is bit-identical"""
    pos = [255, 5, 70, 7, 0] if cap == 256 else [7, 5, 2, 7, 0]     # slots 4, 0, 2 step; 1 and 3 do not
    err, _, _ = _case(dev, H, D, cap, 5, [4, 0, 2], pos, window, poison=True)
    assert err <= BOUND, err


@pytest.mark.parametrize('H,D,cap,pos', [(4, 384, 256, 0), (4, 384, 256, 16), (4, 384, 256, 64), (4, 384, 256, 255),
                                         (1, 8, 8, 7)])
def test_step_footprint_single_row(dev, H, D, cap, pos):
    for window in (0, 3):
        err, _, _ = _case(dev, H, D, cap, 2, [0], [pos, 1], window, poison=True)
        assert err <= BOUND, err


def test_successive_steps_reproduce_the_full_kernel(dev):
    """L = 9 steps, pos bumped by the caller after each, against the rows of ococc_temporal_attention_fwd_f32 under the
    causal mask: within 4e-6, the sum of the two kernels' 2e-6 bounds against float64"""
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ.layers import _TemporalAttention
    B, H, D, Lq, cap = 2, 4, 384, 9, 16
    E = H * D
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(Lq * B, E, generator=g).to(dev) for _ in range(3))     # token-major rows l * B + b
    mask = torch.triu(torch.ones(Lq, Lq, dtype=torch.bool, device=dev), 1)
    full = _TemporalAttention.apply(q, k, v, mask.view(torch.uint8), None, (B, H, Lq, Lq, D), 0.0, None)
    kc, vc = (torch.full((B, cap, E), float('nan'), device=dev) for _ in range(2))
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    slot = torch.tensor([1, 0], dtype=torch.int32, device=dev)                    # row i of a step is tracklet slot[i]
    rows = []
    for l in range(Lq):
        take = l * B + slot.long()
        out = torch.empty(B, E, device=dev)
        L.check(_launch(q[take].contiguous(), k[take].contiguous(), v[take].contiguous(), slot, pos, kc, vc, H, D, -1, out),
                'temporal_attention_step')
        pos += 1
        rows.append(out[slot.long().argsort()])
    steps = torch.stack(rows, 0).view(Lq * B, E)
    err = float((steps.double() - full.double()).abs().max() / full.double().abs().max())
    print(f'steps against the full kernel: {err:.3e}')
    assert err <= 4e-6, err
    assert torch.equal(kc[:, :Lq].transpose(0, 1).reshape(Lq * B, E), k)          # the cache holds the keys, in order


@pytest.mark.parametrize('cap,D', [(257, 8), (8, 6)])
def test_invalid_arguments_launch_nothing(dev, cap, D):
    from objectcentricocccompletion_amd import _lib as L
    H, E = 2, 2 * D
    q = torch.randn(1, 16, device=dev)
    kc, vc = torch.randn(1, cap, E, device=dev), torch.randn(1, cap, E, device=dev)
    out = torch.full((1, 16), 7.0, device=dev)
    keep = (kc.clone(), vc.clone(), out.clone())
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _launch(q, q, q, zero, zero, kc, vc, H, D, 0, out)
    assert rc != 0
    with pytest.raises(L.OcoccError):
        L.check(rc, 'temporal_attention_step')
    torch.cuda.synchronize()
    assert torch.equal(kc, keep[0]) and torch.equal(vc, keep[1]) and torch.equal(out, keep[2])
