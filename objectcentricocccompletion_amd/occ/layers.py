"""Temporal transformer pieces -- host mirror of mmdet3d/models/occ/layers.py:
PositionalEncoding (:8-32), SimpleEncoderLayer (:35-87), TransformerEncoder (:89-99).  (The reference file also holds
a TransformerDecoder / SimpleDecoderLayer that nothing in ococcnet.py instantiates: not on the path, not built.)
Parameter names match nn.MultiheadAttention / the reference (self_attn.in_proj_weight, ...,
linear1, linear2, norm1, norm2) so checkpoints load."""
import copy
import math

import torch
from torch import nn

import os

from .. import gemm
from ..norm import layer_norm_act
from ..sst.sst_ops import get_activation_layer

# the attention core (scores, masks, softmax, dropout, @ v) as ONE launch per direction: csrc/causal_attn.hip (round 6).
# 0: the operator chain below (bmm, masked_fill, softmax, dropout, bmm)
FUSED_ATTENTION = os.environ.get('OCOCC_FUSED_ATTENTION', '1') == '1'


class _TemporalAttention(torch.autograd.Function):
    """ctx rows [L B, E] = softmax(mask(q k^T / sqrt(D))) v per (tracklet, head): ococc_temporal_attention_{fwd,bwd}_f32.
    q / k / v: f32 token-major [L B, H D] (q and k may be column slices of one projection); masks: uint8 or None;
    seed: a device int64 tensor (dropout; drawn by torch's generator, so a captured graph draws a new one per replay)."""

    @staticmethod
    def forward(ctx, q, k, v, attn_mask, key_pad, dims, p_drop, seed):
        # ``k`` None: ``q`` is the packed projection [L B, 2 H D] = q | k (the encoder layers: one product for both) -- the
        # gradient then leaves as ONE [L B, 2 H D] tensor too, and no slice backward (a zero fill + a copy per half) runs
        from .. import _lib as L
        B, H, Lq, S, D = dims
        ctx.packed = k is None
        if ctx.packed:
            qk = q
            q, k = qk[:, :H * D], qk[:, H * D:]
        out = torch.empty((Lq * B, H * D), dtype=torch.float32, device=q.device)
        probs = torch.empty((B * H, Lq, S), dtype=torch.float32, device=q.device)
        L.check(L.lib.ococc_temporal_attention_fwd_f32(
            q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), L.ptr(attn_mask), L.ptr(key_pad),
            B, H, Lq, S, D, float(D) ** -0.5, float(p_drop), 0, L.ptr(seed), probs.data_ptr(), out.data_ptr(), out.stride(0),
            L.stream()), 'temporal_attention_fwd')
        ctx.save_for_backward(qk if ctx.packed else q, v if ctx.packed else k, v, probs, out, *(() if seed is None else (seed,)))
        ctx.meta = (dims, float(p_drop), seed is not None)
        return out

    @staticmethod
    def backward(ctx, d_out):
        from .. import _lib as L
        q, k, v, probs, out = ctx.saved_tensors[:5]
        dims, p_drop, has_seed = ctx.meta
        seed = ctx.saved_tensors[5] if has_seed else None
        B, H, Lq, S, D = dims
        d_out = d_out.contiguous()
        dqk = None
        if ctx.packed:
            qk = q
            q, k = qk[:, :H * D], qk[:, H * D:]
            dqk = torch.empty_like(qk)
            dq, dk = dqk[:, :H * D], dqk[:, H * D:]
        else:
            dq = torch.empty((Lq * B, H * D), dtype=torch.float32, device=q.device)
            dk = torch.empty((S * B, H * D), dtype=torch.float32, device=q.device)
        dv = torch.empty((S * B, H * D), dtype=torch.float32, device=q.device)
        L.check(L.lib.ococc_temporal_attention_bwd_f32(
            q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), B, H, Lq, S, D, float(D) ** -0.5,
            p_drop, 0, L.ptr(seed), probs.data_ptr(), out.data_ptr(), out.stride(0), d_out.data_ptr(), d_out.stride(0),
            dq.data_ptr(), dq.stride(0), dk.data_ptr(), dk.stride(0), dv.data_ptr(), dv.stride(0), L.stream()),
            'temporal_attention_bwd')
        if ctx.packed:
            return dqk, None, dv, None, None, None, None, None
        return dq, dk, dv, None, None, None, None, None


class TemporalCache(object):
    """Keys and values of the frames a tracklet has been stepped through, for online inference (MultiheadAttention.step):
    per encoder layer ``k[i]`` / ``v[i]`` f32 [slots, cap, E] on the device, one slot per tracklet that is being followed.
    ``pos`` int32 [slots] on the device is the number of frames cached per slot, shared by all layers (the attention kernel
    reads it, TransformerEncoder.step bumps it once per step); ``pos_host`` is its mirror on the host, a list of ints, so
    that the bounds checks and ``reset`` need no read-back.

    Memory: 2 * num_layers * cap * E * 4 bytes per slot -- for the ococcnet model (3 layers, E = 1536) at the default
    ``cap`` = 256 (the longest sequence the attention kernels take; the reference's PositionalEncoding stops at 200) that
    is 9.4 MB per slot, 604 MB for 64 slots.  A tracklet longer than ``cap`` frames does not fit: the step raises.

    Past 256 frames (both make the steps call ococc_temporal_attention_step_long_f32):
    ``long``: ``cap`` up to 4096 rows per slot, for a model that attends to all history (151 MB per slot at 4096).
    ``ring``: frame f lives in row f % cap, so a model with test_cfg.attn_window_size = W <= cap, which only ever reads
    the last W frames, follows a tracklet of any length -- a slot is never full (``pos`` is an int32: 2**31 - 1 frames),
    and cap = W = 16 is 0.6 MB per slot.  The step needs 1 <= window <= cap (TransformerEncoder.step checks)."""

    MAX_LONG_CAP, MAX_FRAMES = 4096, 2 ** 31 - 1   # kLongMaxS of csrc/causal_attn_step.hip; the int32 frame counter

    def __init__(self, num_layers, slots, embed_dim, device, cap=256, ring=False, long=False):
        from .. import _lib as L
        device = torch.device(device)   # (a CPU cache can be built and kept account of; every step on it raises)
        self.ring, self.long = bool(ring), bool(long) or bool(ring)
        if self.long:
            if not (1 <= int(cap) <= self.MAX_LONG_CAP):
                raise L.OcoccError(f'TemporalCache: cap {cap} outside 1..{self.MAX_LONG_CAP}, the most frames the long '
                                   'attention step keeps scores for')
        elif not (1 <= int(cap) <= 256):
            raise L.OcoccError(f'TemporalCache: cap {cap} outside 1..256, the longest sequence the attention kernels take')
        if int(slots) < 1 or int(num_layers) < 1:
            raise L.OcoccError('TemporalCache: at least one slot and one layer')
        self.num_layers, self.slots, self.cap, self.embed_dim = int(num_layers), int(slots), int(cap), int(embed_dim)
        self.k = [torch.zeros((self.slots, self.cap, self.embed_dim), dtype=torch.float32, device=device)
                  for _ in range(self.num_layers)]
        self.v = [torch.zeros_like(k) for k in self.k]
        self.pos = torch.zeros((self.slots,), dtype=torch.int32, device=device)
        self.pos_host = [0] * self.slots

    @property
    def device(self):
        return self.pos.device

    def nbytes(self):
        return 2 * self.num_layers * self.slots * self.cap * self.embed_dim * 4

    def check_step(self, slots):
        """the host-side checks of one step over the slot list ``slots``: distinct, and what ``check_steps`` asks of runs
        of one frame -- in range, room for one more frame (a ring cache always has room: only its frame counter can run
        out).  Returns the slots as ints."""
        from .. import _lib as L
        slots = [int(s) for s in slots]
        if len(set(slots)) != len(slots):
            raise L.OcoccError(f'TemporalCache: duplicate slots in one step: {sorted(slots)}')
        return self.check_steps(slots)[0]

    def advance(self, slots, slot_dev):
        """one more frame per ROW of ``slots`` (``slot_dev``: the same list as an int32 / int64 device tensor): a slot
        gains one frame in a step, its run's T_s frames in a chunked step (index_add_ counts a slot once per row it has)"""
        self.pos.index_add_(0, slot_dev.long(), torch.ones_like(slot_dev, dtype=torch.int32))
        for s in slots:
            self.pos_host[s] += 1

    def check_steps(self, slot_rows):
        """the host-side checks of one chunked step (TransformerEncoder.steps) over ``slot_rows``, the slot of every row:
        every slot in range, the rows of a slot consecutive (they are its new frames in order), room for the whole run
        -- pos_host[s] + T_s <= cap, in a ring <= 2**31 - 1.  Returns (slots, offsets, runs): the row list as ints, the
        place 0, 1, 2, ... of each row in its slot's run, and {slot: T_s} in order of appearance.  Modifies nothing."""
        from .. import _lib as L
        slots = [int(s) for s in slot_rows]
        offsets, runs = [], {}
        for i, s in enumerate(slots):
            if not 0 <= s < self.slots:
                raise L.OcoccError(f'TemporalCache: slot {s} outside 0..{self.slots - 1}')
            if s in runs and slots[i - 1] != s:
                raise L.OcoccError(f'TemporalCache: the rows of slot {s} are not consecutive in {slots}: the frames of a '
                                   'slot come as one run, in frame order')
            offsets.append(runs.get(s, 0))
            runs[s] = offsets[-1] + 1
        for s, T in runs.items():
            if self.ring:
                if self.pos_host[s] + T > self.MAX_FRAMES:
                    raise L.OcoccError(f'TemporalCache: {T} more frames take slot {s} from {self.pos_host[s]} past '
                                       '2**31 - 1 frames, the last its int32 counter holds (reset the slot)')
            elif self.pos_host[s] + T > self.cap:
                raise L.OcoccError(f'TemporalCache: slot {s} holds {self.pos_host[s]} frames, {T} more do not fit cap = '
                                   f'{self.cap}; a tracklet longer than the cache is not supported (reset the slot or '
                                   f'build the cache with a larger cap <= {self.MAX_LONG_CAP if self.long else 256})')
        return slots, offsets, runs

    def reset(self, slots=None):
        """forget the frames of ``slots`` (all when None): the slot can follow a new tracklet.  The cached rows are left
        as they are -- nothing reads a row at or past ``pos``."""
        from ..tracklet import host_index
        if slots is None:
            self.pos.zero_()
            self.pos_host = [0] * self.slots
            return
        slots = [int(s) for s in slots]
        for s in slots:
            if not 0 <= s < self.slots:
                from .. import _lib as L
                raise L.OcoccError(f'TemporalCache: slot {s} outside 0..{self.slots - 1}')
        if slots:
            self.pos.index_fill_(0, host_index(slots, self.pos.device), 0)
        for s in slots:
            self.pos_host[s] = 0


def _eval_only(module, what):
    if module.training:
        raise RuntimeError(f'{what} is inference only (no dropout, no backward pass): call .eval() first')


class PositionalEncoding(nn.Module):
    def __init__(self, d_model: int, max_len: int = 200):
        super().__init__()
        self.d_model = d_model
        self.max_len = max_len

    def forward(self, abs_pos):
        """abs_pos [seq_len, batch] -> [seq_len, batch, d_model] = [sin(t w_i) | cos(t w_i)]."""
        div_term = torch.exp(torch.arange(0, self.d_model, 2, device=abs_pos.device)
                             * (-math.log(10000.0) / self.d_model))
        ang = abs_pos[..., None] * div_term
        return torch.cat([torch.sin(ang), torch.cos(ang)], dim=-1)


class MultiheadAttention(nn.Module):
    """Self-attention with the parameter layout of nn.MultiheadAttention (in_proj_weight
    [3E,E], in_proj_bias, out_proj.{weight,bias}); sequence-first tensors [L, B, E].
    Supports the boolean attn_mask / key_padding_mask forms the reference passes.

    Own formulation: q and k share their input (x + pos), so they leave ONE product with the first 2E rows of in_proj
    (the reference's nn.MultiheadAttention runs three), heads are taken as views of that [L B, 2E] result; all products go
    through ``gemm`` (f32 as the reference, or bf16 operands on the matrix cores when gemm.GEMM_DTYPE says so)."""

    def __init__(self, embed_dim, num_heads, dropout=0.0):
        super().__init__()
        assert embed_dim % num_heads == 0
        self.embed_dim, self.num_heads, self.dropout = embed_dim, num_heads, dropout
        self.head_dim = embed_dim // num_heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.out_proj.bias, 0.)

    def _fused_ok(self, q, k, v, L, S, attn_mask, key_padding_mask):
        """the one-launch attention core takes f32 device tensors with 16-byte aligned rows, boolean masks of the shapes
        the reference passes, sequences up to 256 frames (the reference's PositionalEncoding stops at 200), heads up to 384 wide"""
        ok = lambda t: t.is_cuda and t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0
        return (FUSED_ATTENTION and ok(q) and ok(k) and ok(v) and L <= 256 and S <= 256 and self.head_dim % 4 == 0
                and self.head_dim <= 384 and (attn_mask is None or (attn_mask.dtype == torch.bool and attn_mask.shape == (L, S)))
                and (key_padding_mask is None or (key_padding_mask.dtype == torch.bool and key_padding_mask.dim() == 2
                                                  and key_padding_mask.shape[1] == S)))

    def _heads(self, t, n):
        """[n * B, E] token-major -> [B * H, n, D]"""
        return t.reshape(n, -1, self.head_dim).transpose(0, 1)

    def forward(self, query, key, value, attn_mask=None, key_padding_mask=None):
        L, B, E = query.shape
        S = key.shape[0]
        H = self.num_heads
        w, b = self.in_proj_weight, self.in_proj_bias
        if key is query:      # (the encoder layers: q = k = src + pos)
            qk = gemm.linear(query.reshape(L * B, E), w[:2 * E], b[:2 * E])
            q, k = qk[:, :E], qk[:, E:]
        else:
            q = gemm.linear(query.reshape(L * B, E), w[:E], b[:E])
            k = gemm.linear(key.reshape(S * B, E), w[E:2 * E], b[E:2 * E])
        v = gemm.linear(value.reshape(S * B, E), w[2 * E:], b[2 * E:])
        p_drop = self.dropout if self.training else 0.0
        if self._fused_ok(q, k, v, L, S, attn_mask, key_padding_mask):
            am = None if attn_mask is None else attn_mask.contiguous().view(torch.uint8)
            kp = None if key_padding_mask is None else key_padding_mask.contiguous().view(torch.uint8)
            seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=q.device) if p_drop > 0 else None
            packed = key is query and qk.is_contiguous()
            ctx = _TemporalAttention.apply(qk if packed else q, None if packed else k, v, am, kp, (B, H, L, S, self.head_dim),
                                           p_drop, seed)
            return gemm.linear(ctx, self.out_proj.weight, self.out_proj.bias).view(L, B, E), None
        scores = gemm.bmm(self._heads(q * (self.head_dim ** -0.5), L), self._heads(k, S).transpose(1, 2))   # [B H, L, S]
        if attn_mask is not None:
            scores = scores.masked_fill(attn_mask[None], float('-inf')) if attn_mask.dtype == torch.bool \
                else scores + attn_mask[None]
        if key_padding_mask is not None:
            scores = scores.view(B, H, L, S).masked_fill(key_padding_mask[:, None, None, :], float('-inf')).view(B * H, L, S)
        prob = torch.softmax(scores, dim=-1)
        if self.dropout > 0 and self.training:
            prob = torch.nn.functional.dropout(prob, self.dropout)
        ctx = gemm.bmm(prob, self._heads(v, S)).transpose(0, 1).reshape(L * B, E)
        return gemm.linear(ctx, self.out_proj.weight, self.out_proj.bias).view(L, B, E), None

    def _step(self, what, x_qk, x_v, slot, off, cache_k, cache_v, pos, window, ring, long):
        """the body of ``step`` (``off`` None) and ``steps``: the checks, the two in-projections, the attention export
        that (off, long or ring) pick, out_proj"""
        from .. import _lib as L
        _eval_only(self, f'MultiheadAttention.{what}')
        rows = (slot,) if off is None else (slot, off)
        L.require_device(x_qk, x_v, *rows, cache_k, cache_v, pos)
        n, E = x_qk.shape
        assert E == self.embed_dim and x_v.shape == (n, E) and all(r.shape == (n,) and r.dtype == torch.int32 for r in rows)
        assert pos.dtype == torch.int32 and cache_k.shape == cache_v.shape and cache_k.shape[2] == E
        assert cache_k.dtype == cache_v.dtype == torch.float32 and cache_k.is_contiguous() and cache_v.is_contiguous()
        assert pos.shape == (cache_k.shape[0],)
        w, b = self.in_proj_weight, self.in_proj_bias
        qk = gemm.linear(x_qk.float(), w[:2 * E], b[:2 * E])
        v = gemm.linear(x_v.float(), w[2 * E:], b[2 * E:])
        q, k = qk[:, :E], qk[:, E:]
        ctx = torch.empty((n, E), dtype=torch.float32, device=qk.device)
        new = (q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), *(r.data_ptr() for r in rows))
        cached = (pos.data_ptr(), cache_k.data_ptr(), cache_v.data_ptr(), n, cache_k.shape[0], cache_k.shape[1], self.num_heads,
                  self.head_dim, float(self.head_dim) ** -0.5, int(window))
        out = (ctx.data_ptr(), ctx.stride(0), L.stream())
        if off is not None:
            L.check(L.lib.ococc_temporal_attention_chunk_f32(*new, *cached, int(bool(ring)), *out), 'temporal_attention_chunk')
        elif long or ring:
            L.check(L.lib.ococc_temporal_attention_step_long_f32(*new, *cached, int(bool(ring)), *out),
                    'temporal_attention_step_long')
        else:
            L.check(L.lib.ococc_temporal_attention_step_f32(*new, *cached, *out), 'temporal_attention_step')
        return gemm.linear(ctx, self.out_proj.weight, self.out_proj.bias)

    @torch.no_grad()
    def step(self, x_qk, x_v, slot, cache_k, cache_v, pos, window=-1, ring=False, long=False):
        """One new frame per tracklet against the cached ones: x_qk, x_v [n, E] (this frame's src + pos and src),
        ``slot`` int32 [n] the cache slot of each row, cache_k / cache_v [slots, cap, E] this layer's cache, ``pos`` int32
        [slots] the frames cached per slot.  q and k leave one product with the first 2E rows of in_proj as in ``forward``;
        ococc_temporal_attention_step_f32 appends k and v at row pos[slot] and attends to the frames lo..pos[slot]
        (``window`` > 0: the last ``window`` frames, as get_future_mask windows the past); out_proj follows.  ``pos`` is
        left as it is.  ``long`` / ``ring`` (TemporalCache): ococc_temporal_attention_step_long_f32 instead -- caches of up
        to 4096 rows, and with ``ring`` frame f in row f % cap (1 <= window <= cap).  No fall-back: arguments the kernel
        does not take raise."""
        return self._step('step', x_qk, x_v, slot, None, cache_k, cache_v, pos, window, ring, long)

    @torch.no_grad()
    def steps(self, x_qk, x_v, slot, off, cache_k, cache_v, pos, window=-1, ring=False):
        """``step`` for one OR MORE new frames per tracklet in one launch (ococc_temporal_attention_chunk_f32): the rows
        of a slot are consecutive and in frame order, ``off`` int32 [n] the place 0, 1, 2, ... of each row in its slot's
        run (TemporalCache.check_steps).  Row i is frame pos[slot] + off[i]: it attends to the cached frames and to the
        earlier rows of its own run; the keys and values of all rows are appended afterwards, inside the same call.  The
        export picks the instance by cap and ``ring`` itself.  ``pos`` is left as it is."""
        return self._step('steps', x_qk, x_v, slot, off, cache_k, cache_v, pos, window, ring, False)


class SimpleEncoderLayer(nn.Module):
    """Post-LN encoder layer with q = k = src + pos, v = src (layers.py:35-87): attention block, then feed-forward block,
    each `x <- LayerNorm(x + dropout(block(x)))` with the LayerNorm on the HIP kernel."""

    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation='gelu', mlp_dropout=0):
        super().__init__()
        self.self_attn = MultiheadAttention(d_model, nhead, dropout)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(mlp_dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.dropout1 = nn.Dropout(mlp_dropout)
        self.dropout2 = nn.Dropout(mlp_dropout)
        self.activation = get_activation_layer(activation)
        self.fp16_enabled = False

    def with_pos_embed(self, tensor, pos):
        return tensor if pos is None else tensor + pos

    def _residual_norm(self, norm, x, branch, drop):
        return layer_norm_act(x + drop(branch), norm.weight, norm.bias, norm.eps, 'none')   # nn.LayerNorm parameters, HIP kernel

    def _feed_forward(self, x):
        hidden = self.dropout(self.activation(gemm.linear(x, self.linear1.weight, self.linear1.bias)))
        return gemm.linear(hidden, self.linear2.weight, self.linear2.bias)

    def _after_attention(self, src, attended):
        x = self._residual_norm(self.norm1, src, attended, self.dropout1)
        return self._residual_norm(self.norm2, x, self._feed_forward(x), self.dropout2)

    def forward(self, src, key_padding_mask=None, pos_enc=None, attn_mask=None):
        qk_in = self.with_pos_embed(src, pos_enc)
        attended, _ = self.self_attn(qk_in, qk_in, value=src, attn_mask=attn_mask, key_padding_mask=key_padding_mask)
        return self._after_attention(src, attended)

    @torch.no_grad()
    def step(self, src, pos_enc, slot, cache_k, cache_v, pos, window=-1, ring=False, long=False):
        """``forward`` for one new frame per tracklet, src / pos_enc [n, E], against this layer's cache
        (MultiheadAttention.step, which ``ring`` / ``long`` go to): the same post-LN structure, the dropouts are the
        identity (inference only)."""
        _eval_only(self, 'SimpleEncoderLayer.step')
        return self._after_attention(src, self.self_attn.step(self.with_pos_embed(src, pos_enc), src, slot, cache_k, cache_v,
                                                              pos, window, ring, long))

    @torch.no_grad()
    def steps(self, src, pos_enc, slot, off, cache_k, cache_v, pos, window=-1, ring=False):
        """``step`` for one or more new frames per tracklet (MultiheadAttention.steps): everything but the attention
        works per row"""
        _eval_only(self, 'SimpleEncoderLayer.steps')
        return self._after_attention(src, self.self_attn.steps(self.with_pos_embed(src, pos_enc), src, slot, off, cache_k,
                                                               cache_v, pos, window, ring))


def _get_clones(module, N):
    return nn.ModuleList([copy.deepcopy(module) for _ in range(N)])


class TransformerEncoder(nn.Module):
    """``num_layers`` copies of an encoder layer applied in turn (layers.py:89-99; parameter names layers.<i>....)"""

    def __init__(self, encoder_layer, num_layers):
        super().__init__()
        self.layers = _get_clones(encoder_layer, num_layers)
        self.num_layers = num_layers

    def forward(self, src, key_padding_mask=None, pos_enc=None, attn_mask=None):
        x = src
        for layer in self.layers:
            x = layer(x, key_padding_mask=key_padding_mask, pos_enc=pos_enc, attn_mask=attn_mask)
        return x

    def _step(self, src, pos_enc, slots, offsets, cache, window):
        """the body of ``step`` (``offsets`` None) and ``steps`` over rows that the cache has checked: the checks of the
        cache against this encoder and the rows, ONE upload of the row indices, the layers in turn, one bump"""
        from .. import _lib as L
        from ..tracklet import host_index
        if cache.num_layers != self.num_layers:
            raise L.OcoccError(f'TemporalCache of {cache.num_layers} layers for an encoder of {self.num_layers}')
        ring, long = cache.ring, cache.long
        if ring and not 1 <= int(window) <= cache.cap:
            raise L.OcoccError(f'a ring TemporalCache of cap = {cache.cap} rows serves windows of 1..{cache.cap} frames, not '
                               f'window = {window}: the row of frame t overwrites frame t - cap')
        if len(slots) != src.shape[0]:
            raise L.OcoccError(f'{len(slots)} slots for {src.shape[0]} rows')
        L.require_device(src, pos_enc, cache.pos)
        rows = host_index(slots + (offsets or []), src.device, dtype=torch.int32)   # (slots | offsets: one upload)
        slot_dev, off_dev = rows[:len(slots)], rows[len(slots):]
        x = src
        for i, layer in enumerate(self.layers):
            if offsets is None:
                x = layer.step(x, pos_enc, slot_dev, cache.k[i], cache.v[i], cache.pos, window, ring, long)
            else:
                x = layer.steps(x, pos_enc, slot_dev, off_dev, cache.k[i], cache.v[i], cache.pos, window, ring)
        cache.advance(slots, slot_dev)
        return x

    @torch.no_grad()
    def step(self, src, pos_enc, slot, cache, window=-1):
        """One new frame for each of n tracklets: src, pos_enc [n, E]; ``slot``: the cache slot of each row, a list of
        ints (a tensor is read back: the bounds checks run on the host); ``cache`` a TemporalCache with one (k, v) pair
        per layer.  Row i equals row pos[slot[i]] of ``forward`` over the frames 0..pos[slot[i]] of that tracklet under the
        future mask (windowed by ``window`` > 0).  Bumps ``cache.pos`` and its host mirror once, after the last layer.
        A ring cache (``cache.ring``) needs 1 <= window <= cache.cap.
        The host-side checks (duplicate slots, a step past ``cache.cap``, a window a ring cache cannot serve, CPU tensors)
        raise before anything is launched."""
        _eval_only(self, 'TransformerEncoder.step')
        slots = cache.check_step(slot.tolist() if torch.is_tensor(slot) else slot)
        return self._step(src, pos_enc, slots, None, cache, window)

    @torch.no_grad()
    def steps(self, src, pos_enc, slot_rows, cache, window=-1):
        """One or more new frames for each of several tracklets in one call: src, pos_enc [n, E], one row per (tracklet,
        frame); ``slot_rows``: the cache slot of each row, a list of ints (a tensor is read back), the rows of a slot
        consecutive and in frame order -- [3, 3, 3, 0, 5, 5] gives slot 3 three frames, slot 0 one, slot 5 two.  Row j of
        the run of slot s equals row pos[s] + j of ``forward`` over the frames 0..pos[s] + j of that tracklet under the
        future mask (windowed by ``window`` > 0).  Every layer is one attention launch and one append launch whatever n
        is; a ring cache takes runs longer than its cap.  Bumps ``cache.pos`` and its host mirror by the runs once, after
        the last layer.  The host-side checks (a window a ring cache cannot serve, slots out of range, rows of a slot that
        are not consecutive, a run past ``cache.cap``, CPU tensors) raise before anything is launched."""
        _eval_only(self, 'TransformerEncoder.steps')
        slots, offsets, _ = cache.check_steps(slot_rows.tolist() if torch.is_tensor(slot_rows) else slot_rows)
        return self._step(src, pos_enc, slots, offsets, cache, window)
