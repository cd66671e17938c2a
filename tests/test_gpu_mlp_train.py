"""What the decoder's TRAINING launch stores (csrc/mlp_layer.hip, occ_mlp_fwd_kernel<DROP, TRAIN = true>, reached as
ococc_occ_mlp_train_fwd_bf16): per layer the LayerNorm input z (bf16), the row statistics and the activation y, besides
the logits -- each against float64 (oracle/decoder_ref.py, rounding='train') taken from the layer's STORED input, so
that errors do not compound and one wrong row shows; and the gradients fused_mlp.occ_mlp_train hands back against
float64 autograd through the same forward."""
import ctypes

import pytest
import torch

from oracle import decoder_ref as D

pytestmark = pytest.mark.gpu
U = 2.0 ** -24          # unit round-off of f32
BF16_ULP = 2.0 ** -7    # one step of a bf16 value v is at most 2^-7 |v|
EPS = 1e-3
WIDTHS = (512, 1024, 1024)
PE_COLS = 60            # 6 L columns of the positional encoding; the kernel's operand is padded to 64 (zeros)
PAD = 64                # extra rows behind every output buffer
SENT16, SENT32 = 0x5A3C, 0x4B1D2C3E   # bf16 / f32 bit patterns (1.3e16, 1.03e7): fixed, non-zero, nothing the kernel computes
THR = 6554              # round(0.1 * 65536)
SEEDS = [11, 2 ** 40 + 5, 77]
ROIS, EMPTY_ROI = 7, 3  # roi_part rows; no query row points at row 3


def second_trip_rows(dev):
    """(rows, CU count): 64 (CU + 1) + 27 rows = CU + 2 tiles on a grid of CU workgroups -- two workgroups go through
    the tile loop a second time, one of them into the ragged 27-row tile."""
    cu = torch.cuda.get_device_properties(dev).multi_processor_count
    return 64 * (cu + 1) + 27, cu


def make_inputs(dev, rows):
    g = torch.Generator().manual_seed(rows)
    W = [torch.randn(n, k, generator=g) / k ** 0.5 for k, n in ((PE_COLS, 512), (512, 1024), (1024, 1024))]
    gam = [1 + 0.2 * torch.randn(n, generator=g) for n in WIDTHS]
    bet = [0.2 * torch.randn(n, generator=g) for n in WIDTHS]
    hw, hb = torch.randn(1, 1024, generator=g) / 32, torch.tensor([-0.1])
    xyz = (torch.rand(rows, 3, generator=g) * 2 - 1) * torch.tensor([8., 8., 4.])
    add = torch.randn(ROIS, 512, generator=g)
    idx = torch.randint(0, ROIS - 1, (rows,), generator=g).sort().values   # non-decreasing, as the decoder's queries are
    idx = (idx + (idx >= EMPTY_ROI)).int()
    from objectcentricocccompletion_amd.occ import fused_mlp as fm
    to = lambda t: t.to(dev)
    inp = dict(W=[to(w) for w in W], gam=[to(t) for t in gam], bet=[to(t) for t in bet], hw=to(hw), hb=to(hb), add=to(add),
               idx=to(idx), rows=rows)
    inp['pe'] = fm.pos_encode_bf16(to(xyz), 10, [-8.0, -8.0, -4.0, 8.0, 8.0, 4.0])
    return inp


def launch(inp, thr, seeds):
    """ococc_occ_mlp_train_fwd_bf16 into buffers of rows + PAD rows prefilled with the sentinel -> dict of the whole
    buffers z[3], y[3] (bf16), stats[3] (f32 [., 2]), out (f32)."""
    from objectcentricocccompletion_amd import _lib as L
    from objectcentricocccompletion_amd.occ import fused_mlp as fm
    rows, dev = inp['rows'], inp['pe'].device
    frags = fm.linear_fragments32(inp['W'], [64, 512, 1024])
    b16 = lambda n: torch.full((rows + PAD, n), SENT16, dtype=torch.int16, device=dev).view(torch.bfloat16)
    f32 = lambda *s: torch.full(s, SENT32, dtype=torch.int32, device=dev).view(torch.float32)
    o = dict(z=[b16(n) for n in WIDTHS], y=[b16(n) for n in WIDTHS], stats=[f32(rows + PAD, 2) for _ in WIDTHS],
             out=f32(rows + PAD))
    vp = lambda ts: (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts])
    sd = (ctypes.c_uint64 * 3)(*seeds) if thr else None
    L.check(L.lib.ococc_occ_mlp_train_fwd_bf16(
        L.ptr(inp['pe']), rows, L.ptr(inp['add']), L.ptr(inp['idx']), vp(frags), vp(inp['gam']), vp(inp['bet']), EPS,
        L.ptr(inp['hw']), L.ptr(inp['hb']), thr, sd, vp(o['z']), vp(o['y']), vp(o['stats']), L.ptr(o['out']), L.stream()),
        'occ_mlp_train_fwd')
    torch.cuda.synchronize()
    return o


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for k in ('z', 'y', 'stats') for x, y in zip(a[k], b[k])) and \
        torch.equal(bits(a['out']), bits(b['out']))


def keep_mask(z, y, gam, bet, thr, seed, what):
    """The mask the launch applied to y (stored, [rows, n]) is the one the LayerNorm kernels -- forward here, hence their
    backward, which regenerates it from the same (threshold, seed) -- apply to the stored z.  -> keep (bool) for the
    float64 reference, or None without dropout."""
    from objectcentricocccompletion_amd.norm import _LayerNormAct
    ref0 = _LayerNormAct.apply(z, gam, bet, EPS, 1)
    e0 = D.train_act(z, gam, bet, EPS)
    live = (ref0 != 0) & (e0 != 0)   # non-zero undropped on both sides (the kernel's side: the float64 value of its z)
    share = float(live.double().mean())
    assert share >= 0.999, (what, share)
    if not thr:
        assert not bool(((y == 0) & live).any()), what
        return None
    ref = _LayerNormAct.apply(z, gam, bet, EPS, 1, thr, seed)
    dropped = (y == 0) & live
    assert torch.equal(dropped, (ref == 0) & live), what
    n, p = float(live.sum()), thr / 65536.0
    frac = float(dropped.sum()) / n
    print(f'{what}: live {share:.5f}, dropped {frac:.5f} (p = {p:.5f}, sigma {(p * (1 - p) / n) ** 0.5:.2e})')
    assert abs(frac - p) <= 5 * (p * (1 - p) / n) ** 0.5, (what, frac)
    return ~dropped


def check_layer(l, x, inp, o, thr, seed):
    """Layer l of a launch against float64 of its stored input x (bf16 [rows, k])."""
    rows, n = inp['rows'], WIDTHS[l]
    W, gam, bet = inp['W'][l], inp['gam'][l], inp['bet'][l]
    z, y, st = o['z'][l][:rows], o['y'][l][:rows], o['stats'][l][:rows].double()
    what = f'layer {l} rows {rows} thr {thr}'
    # z = r16(x r16(W)^T [+ roi_part[idx]]): a bf16 store behind an f32 accumulation -- equal to the float64 value's
    # rounding, or (f32 sums near a rounding boundary) its neighbour
    ez = D.mlp_layer(x, W, gam, bet, EPS, add=inp['add'] if l == 0 else None, idx=inp['idx'] if l == 0 else None,
                     rounding='train')[2]
    dz = (z.double() - ez).abs()
    eq = float((dz == 0).double().mean())
    print(f'{what}: z largest error {float(dz.max()):.3e}, equal {eq:.4f}')
    assert bool((dz <= BF16_ULP * (ez.abs() + 0.05) + 1e-6).all()), (what, float(dz.max()))
    assert eq > 0.97, (what, eq)
    # statistics: those of the STORED (rounded) z, in float64.  Any order of f32 summation of N numbers satisfies
    #   |fl(sum) - sum| <= (N - 1) u sum |x_i|,  u = 2^-24;
    # mean = fl(fl(sum) / N): one more rounding, so  |mean - mean64| <= N u mean_c |z| =: Em.
    # The kernel then sums fl(fl(z_i - mean)^2): three roundings per term and N - 1 of the summation, and
    # sum_i (z_i - mean)^2 = sum_i (z_i - mean64)^2 + N (mean - mean64)^2 exactly; the division by N, eps as an f32 and
    # the addition are three more.  With v = var64 + eps:  |v^ - v| <= (N + 5) u v + Em^2 =: rv v,  and
    # rstd = rsqrtf(v^) (one ulp = 2^-23 relative):  |rstd - rstd64| <= rstd64 (rv / 2 + rv^2 + 2^-23).
    zd = z.double()
    m64, r64 = D.ln_stats(zd, EPS)
    em = n * U * zd.abs().mean(-1)
    rv = (n + 5) * U + em ** 2 * r64 ** 2
    er = r64 * (0.5 * rv + rv ** 2 + 2.0 ** -23)
    dm, dr = (st[:, 0] - m64).abs(), (st[:, 1] - r64).abs()
    print(f'{what}: mean largest error {float(dm.max()):.3e} (largest error / bound {float((dm / em).max()):.4f}), '
          f'rstd {float(dr.max()):.3e} ({float((dr / er).max()):.4f})')
    assert bool((dm <= em).all()), (what, float((dm / em).max()))
    assert bool((dr <= er).all()), (what, float((dr / er).max()))
    # dropout mask, then y = r16(keep scale GELU(LN64(stored z))), one rounding behind f32 arithmetic as above
    keep = keep_mask(z, y, gam, bet, thr, seed, what)
    scale = 65536.0 / (65536.0 - thr)
    ey = D.train_act(zd, gam, bet, EPS, keep, thr)
    dy = (y.double() - ey).abs()
    eq = float((dy == 0).double().mean())
    print(f'{what}: y largest error {float(dy.max()):.3e}, equal {eq:.4f}')
    assert bool((dy <= BF16_ULP * (ey.abs() + 0.05 * scale) + 1e-6).all()), (what, float(dy.max()))
    assert eq > 0.97, (what, eq)
    return keep


CASES = [1, 63, 64, 65, None]   # None: second_trip_rows


@pytest.mark.parametrize('thr', [0, THR])
@pytest.mark.parametrize('rows', CASES, ids=lambda r: 'second-trip' if r is None else str(r))
def test_train_launch_stores(dev, rows, thr):
    if rows is None:
        rows, cu = second_trip_rows(dev)
        assert (rows + 63) // 64 > cu and rows % 64 == 27   # the persistent loop's second trip runs, ragged tile included
    inp = make_inputs(dev, rows)
    o = launch(inp, thr, SEEDS)
    x = inp['pe'][:, :PE_COLS]
    for l in range(3):
        check_layer(l, x, inp, o, thr, SEEDS[l])
        x = o['y'][l][:rows]
    # logits: the f32 dot product of the stored y2 with the head's weights, 1024 terms
    y2, hw = o['y'][2][:rows].double(), inp['hw'].double().view(-1)
    e = y2 @ hw + inp['hb'].double().view(())
    bound = 1024 * U * (y2.abs() @ hw.abs()) + 1e-7
    d = (o['out'][:rows].double() - e).abs()
    print(f'rows {rows} thr {thr}: logits largest error {float(d.max()):.3e} (largest error / bound {float((d / bound).max()):.4f})')
    assert bool((d <= bound).all()), float((d / bound).max())
    # nothing is written behind the last row
    for k in ('z', 'y', 'stats'):
        for t in o[k]:
            assert bool((bits(t[rows:]) == (SENT16 if t.dtype == torch.bfloat16 else SENT32)).all()), k
    assert bool((bits(o['out'][rows:]) == SENT32).all())
    # the same seeds: the same bits everywhere; other seeds: other masks
    assert same_bits(o, launch(inp, thr, SEEDS))
    if thr:
        other = launch(inp, thr, [s + 1 for s in SEEDS])
        for l in range(3):
            assert not torch.equal(other['y'][l][:rows] == 0, o['y'][l][:rows] == 0), l


# ---------------------------------------------------------------------------------------------------------------------
# Gradients.  err = |g - g64| / |g64| norm-wise, g64 from float64 autograd through the oracle's 'train' forward (roundings
# straight-through, the launch's own keep masks); the fused step (one-launch forward + backward chain) against the
# operator-by-operator bf16 chain it replaces (OccDecoder.forward with FUSED_TRAIN_MLP off: f32 first-layer GEMM, LayerNorm
# kernels, library GEMMs under autocast), same seeds: err_fused <= 1.5 err_operator + 2e-3, as
# test_fused_decoder_training_step asks against the f32 decoder.  Measured on MI355X, err_fused / err_operator:
#                 rows 65, p = 0       rows 65, p = 0.1     rows 2331, p = 0     rows 2331, p = 0.1
#   (logits)      9.6e-4 / 1.0e-2      8.6e-4 / 6.9e-3      4.8e-4 / 5.7e-3      4.6e-4 / 5.7e-3
#   roi_part      5.9e-3 / 7.7e-3      5.2e-3 / 6.7e-3      5.4e-3 / 7.3e-3      5.3e-3 / 7.1e-3
#   W_pe          4.7e-3 / 6.0e-3      4.6e-3 / 5.9e-3      4.8e-3 / 6.2e-3      4.8e-3 / 6.2e-3
#   W1            5.1e-3 / 7.6e-3      4.7e-3 / 6.7e-3      4.9e-3 / 7.1e-3      4.8e-3 / 6.9e-3
#   W2            4.5e-3 / 8.1e-3      4.1e-3 / 7.0e-3      3.9e-3 / 7.1e-3      3.9e-3 / 6.6e-3
#   g0, b0        5.4e-3, 5.9e-3 /     5.0e-3, 4.9e-3 /     4.4e-3, 4.6e-3 /     4.6e-3, 4.6e-3 /
#                 8.0e-3, 8.3e-3       6.8e-3, 6.4e-3       6.3e-3, 6.0e-3       6.4e-3, 6.5e-3
#   g1, b1        5.2e-3, 5.8e-3 /     4.5e-3, 4.6e-3 /     4.0e-3, 4.0e-3 /     4.0e-3, 4.1e-3 /
#                 8.4e-3, 8.6e-3       7.0e-3, 6.7e-3       6.5e-3, 5.8e-3       6.3e-3, 6.0e-3
#   g2, b2        4.3e-3, 4.8e-3 /     3.8e-3, 4.1e-3 /     2.9e-3, 2.7e-3 /     3.0e-3, 2.8e-3 /
#                 8.8e-3, 8.3e-3       7.5e-3, 6.5e-3       6.8e-3, 4.6e-3       5.8e-3, 4.5e-3
#   head_w        3.3e-3 / 8.9e-3      2.7e-3 / 7.6e-3      2.2e-3 / 6.9e-3      2.3e-3 / 6.1e-3
#   head_b        3.0e-5 / 1.5         3.0e-5 / 1.5         9.3e-9 / 6.8e-5      9.3e-9 / 6.8e-5
# (head_b: the sum of dlogit -- f32 in the fused step, a bf16 sum of bf16 values in the operator chain, and 65 random
# numbers nearly cancel.)  Every fused gradient is closer to float64 than the operator chain's.
NAMES = ('roi_part', 'W_pe', 'W1', 'W2', 'g0', 'b0', 'g1', 'b1', 'g2', 'b2', 'head_w', 'head_b')


def leaves(inp, dtype):
    src = [inp['add'], *inp['W'], inp['gam'][0], inp['bet'][0], inp['gam'][1], inp['bet'][1], inp['gam'][2], inp['bet'][2],
           inp['hw'], inp['hb']]
    return {k: t.detach().to(dtype).clone().requires_grad_(True) for k, t in zip(NAMES, src)}


@pytest.mark.parametrize('dropout', [0.0, 0.1])
@pytest.mark.parametrize('rows', [65, 2331])
def test_train_gradients_vs_float64(dev, rows, dropout):
    from objectcentricocccompletion_amd.occ import fused_mlp as fm
    from objectcentricocccompletion_amd.linear import tall_addmm
    from objectcentricocccompletion_amd.norm import _LayerNormAct
    from objectcentricocccompletion_amd.voxel.scatter_points import gather_rows
    inp = make_inputs(dev, rows)
    thr = int(round(dropout * 65536))
    assert thr in (0, THR)
    pe, idx = inp['pe'], inp['idx']
    g = torch.Generator().manual_seed(5)
    dl = torch.randn(rows, 1, generator=g).to(dev)
    # fused step
    p = leaves(inp, torch.float32)
    out_f = fm.occ_mlp_train(pe, p['roi_part'], idx, p['W_pe'], p['W1'], p['W2'], [p['g0'], p['g1'], p['g2']],
                             [p['b0'], p['b1'], p['b2']], EPS, p['head_w'], p['head_b'], thr, SEEDS, fm.DecoderWeights())
    out_f.backward(dl)
    torch.cuda.synchronize()
    fused = {k: v.grad.double() for k, v in p.items()}
    # the masks of that forward: the export with the same inputs (bit-identical launch), checked against the LayerNorm kernels
    o = launch(inp, thr, SEEDS)
    assert torch.equal(o['out'][:rows], out_f.detach().view(-1))
    keeps = [keep_mask(o['z'][l][:rows], o['y'][l][:rows], inp['gam'][l], inp['bet'][l], thr, SEEDS[l], f'layer {l}')
             for l in range(3)]
    # float64 reference
    q = leaves(inp, torch.float64)
    x, head = pe[:, :PE_COLS], None
    for l, (w, ga, be) in enumerate((('W_pe', 'g0', 'b0'), ('W1', 'g1', 'b1'), ('W2', 'g2', 'b2'))):
        x, head = D.mlp_layer(x, q[w], q[ga], q[be], EPS, add=q['roi_part'] if l == 0 else None, idx=idx if l == 0 else None,
                              head_w=q['head_w'] if l == 2 else None, head_b=q['head_b'] if l == 2 else None,
                              rounding='train', keep=keeps[l], drop_threshold=thr)[:2]
    head.backward(dl.double().view(-1))
    ref = {k: v.grad for k, v in q.items()}
    # operator-by-operator bf16 chain
    r = leaves(inp, torch.float32)
    h = tall_addmm(gather_rows(r['roi_part'], idx.long()), pe[:, :PE_COLS].float(), r['W_pe']).to(torch.bfloat16)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        for l, (ga, be, w) in enumerate((('g0', 'b0', 'W1'), ('g1', 'b1', 'W2'), ('g2', 'b2', 'head_w'))):
            h = _LayerNormAct.apply(h, r[ga], r[be], EPS, 1, thr, SEEDS[l]) if thr else _LayerNormAct.apply(h, r[ga], r[be], EPS, 1)
            h = torch.nn.functional.linear(h, r[w], r['head_b'] if l == 2 else None)
    out_o = h.float()
    out_o.backward(dl)
    torch.cuda.synchronize()
    oper = {k: v.grad.double() for k, v in r.items()}
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp(min=1e-300))
    hd = head.detach()
    print(f'rows {rows} dropout {dropout}: logits fused {rel(out_f.detach().double().view(-1), hd):.2e} '
          f'operator {rel(out_o.detach().double().view(-1), hd):.2e}')
    bad = []
    for k in NAMES:
        assert ref[k].shape == fused[k].shape == oper[k].shape and float(ref[k].norm()) > 0, k
        ef, eo = rel(fused[k], ref[k]), rel(oper[k], ref[k])
        print(f'  d {k:9s} fused {ef:.2e}  operator {eo:.2e}')
        if not ef <= 1.5 * eo + 2e-3:
            bad.append((k, ef, eo))
    assert not bad, bad
    # no query points at this RoI: no gradient reaches its row
    assert bool((p['roi_part'].grad[EMPTY_ROI] == 0).all()) and bool((ref['roi_part'][EMPTY_ROI] == 0).all())
    assert not bool((idx == EMPTY_ROI).any())
