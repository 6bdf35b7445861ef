"""Backend-stub decode ops: HIP kernels (``_hipops``) and plain-PyTorch fp32
reference implementations of the same math (used by the numerics tests and,
explicitly requested, by CPU-only engine tests -- never as a silent fallback
on a GPU host).

KV cache layout per layer: ``[slots, kv_heads, max_ctx, 128]`` bf16.
"""
from __future__ import annotations

import math
from typing import Optional

import os

import torch

from .. import _native


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _check(t: torch.Tensor, dtype, name: str):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


class HipOps:
    """Thin validated wrappers over the HIP kernels."""

    def __init__(self):
        self.k = _native.require_hipops()

    def rmsnorm(self, x: torch.Tensor, w: torch.Tensor, eps: float, residual: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        _check(x, torch.bfloat16, "x")
        _check(w, torch.bfloat16, "w")
        T, D = x.shape
        if w.numel() != D:
            raise ValueError("rmsnorm weight size mismatch")
        if residual is not None:
            _check(residual, torch.bfloat16, "residual")
            if residual.shape != x.shape:
                raise ValueError("residual shape mismatch")
        y = out if out is not None else torch.empty_like(x)
        self.k.rmsnorm(x.data_ptr(), residual.data_ptr() if residual is not None else 0, w.data_ptr(),
                       y.data_ptr(), T, D, float(eps), _stream(x))
        return y

    def silu_mul(self, gu: torch.Tensor, out: Optional[torch.Tensor] = None, perm: bool = False) -> torch.Tensor:
        """silu(gate) * up; ``perm``: ``gu`` columns are in the fused GEMM's
        swiglu order (``ops.gemm.swiglu_perm_index``) instead of [gate | up]."""
        _check(gu, torch.bfloat16, "gu")
        T, F2 = gu.shape
        F = F2 // 2
        y = out if out is not None else torch.empty((T, F), dtype=gu.dtype, device=gu.device)
        self.k.silu_mul(gu.data_ptr(), y.data_ptr(), T, F, _stream(gu), perm)
        return y

    def row_rms(self, x: torch.Tensor, eps: float) -> torch.Tensor:
        """1 / sqrt(mean(x^2) + eps) per row (the RMSNorm scale), fp32.  The
        buffer holds ceil(T/256)*256 floats -- the fused GEMMs read whole
        256-row tiles of it with vector loads -- and its first T are the
        scales."""
        from .gemm import row_scale_len
        _check(x, torch.bfloat16, "x")
        T, D = x.shape
        r = torch.empty(row_scale_len(T), dtype=torch.float32, device=x.device)
        self.k.row_rms(x.data_ptr(), r.data_ptr(), T, D, float(eps), _stream(x))
        return r

    def swiglu_rows(self, x, w_perm, r):
        """The MLP up-projection of rmsnorm(x): one GEMM over the raw rows,
        the norm weight folded into ``w_perm``, ``r`` applied per row."""
        from . import gemm as G
        return G.gemm_swiglu(x, w_perm, row_scale=r)

    def qkv_rope_rows(self, x, wqkv, r, pos, slot, cos_t, sin_t, Hq, Hkv, kc, vc, split=True, split_full=None):
        from . import gemm as G
        return G.qkv_rope(x, wqkv, pos, slot, cos_t, sin_t, Hq, Hkv, kc, vc, row_scale=r, split=split,
                          split_full=split_full)

    def greedy_head(self, x, w, fused: bool = True, min_rows: int = 256):
        """Greedy tokens of the LM head (int32 [M]): the hand-written GEMM
        with the argmax epilogue from ``min_rows`` rows (no logits tensor),
        else hipBLASLt + torch.argmax."""
        from . import gemm as G
        if fused and x.shape[0] >= min_rows and G.supported(x.shape[0], w.shape[0], x.shape[1]):
            return G.lm_head_argmax(x, w)
        return torch.argmax(torch.nn.functional.linear(x, w), dim=-1).to(torch.int32)

    def sample_head(self, x, w, inv_temp, keys, fused: bool = True, min_rows: int = 256):
        """Tokens of the LM head under per-row temperature sampling (int32
        [M]; ``ops.gemm.lm_head_sample``): the hand-written GEMM with the
        sampling epilogue from ``min_rows`` rows (no logits tensor), else
        the same scores (fp32 logits * inv_temp + the contract's noise, from
        the device generator) over a logits tensor."""
        from . import gemm as G
        M = x.shape[0]
        if fused and M >= min_rows and G.supported(M, w.shape[0], x.shape[1]):
            return G.lm_head_sample(x, w, inv_temp, keys)
        from .sampling import SERIES_BELOW
        lg = torch.nn.functional.linear(x, w).float()
        m = G.sample_bits(keys[:M].contiguous(), 0, w.shape[0]).to(torch.int64) & 0xFFFFFFFF
        v = (m.double() + 0.5) * 2.0 ** -32
        e = torch.where(v < SERIES_BELOW, v * (1.0 + v * (0.5 + v / 3.0)), -torch.log1p(-v.clamp(min=SERIES_BELOW)))
        it = inv_temp[:M, None]
        sc = torch.where(it != 0, lg.double() * it.double() - torch.log(e), lg.double())
        return torch.argmax(sc, dim=-1).to(torch.int32)

    def _row_logits(self, x, w, entry: str):
        """bf16 logits of the rows ``x`` for a row-wise head, in the grow-only
        scratch entry ``entry``: the 256x256 tile kernel's store epilogue
        whatever the row count -- no split-K, no skinny kernel -- so a row's
        logits are the bf16 rounding of the fp32 accumulators the fused head
        scores and do not depend on who shares the step.  A shape the tile
        kernel refuses takes ``F.linear``, its columns padded to a multiple
        of 8."""
        from . import gemm as G
        R, V = x.shape[0], w.shape[0]
        if G.supported(R, V, x.shape[1]):
            buf, = G._scratch(x.device, _stream(x), entry, (R * V, 0, torch.empty, torch.bfloat16))
            return G.gemm(x.contiguous(), w, out=buf[:R * V].view(R, V))
        lg = torch.nn.functional.linear(x, w)
        if V % 8:
            lg = torch.nn.functional.pad(lg, (0, 8 - V % 8))
        return lg.contiguous()

    def truncated_head(self, x, w, inv_temp, keys, top_k, top_p, log_min_p=None):
        """Tokens of the LM head under top-k / top-p / min-p sampling (int32
        [R]; ``ops.gemm.sample_truncated``; ``log_min_p`` float32 [R] or None:
        ``ops.sampling.min_p_log``) for the rows that ask for it, over their
        own logits (``_row_logits``)."""
        from . import gemm as G
        lg = self._row_logits(x, w, "trunc")
        return G.sample_truncated(lg, inv_temp.contiguous(), keys.contiguous(), top_k, top_p, vocab=w.shape[0],
                                  log_min_p=None if log_min_p is None else log_min_p.contiguous())

    def logprob_head(self, x, w, tok):
        """Log-probabilities of the LM head for the rows that ask for them:
        ``(lp float32 [L][6], ids int32 [L][5])`` of ``ops.gemm.
        token_logprobs`` -- the token ``tok`` (int32 [L]) first, then the 5
        most likely.  The logits are the rows' own (``_row_logits``, a
        scratch entry of their own), so a row's result depends on nothing but
        the row."""
        from . import gemm as G
        lg = self._row_logits(x, w, "logp")
        return G.token_logprobs(lg, tok.to(torch.int32).contiguous(), vocab=w.shape[0])

    def penalised_head(self, x, w, inv_temp, keys, top_k, top_p, hist, spans, params, n_greedy=None, edit=None,
                       log_min_p=None):
        """Tokens of the LM head (int32 [R]) for the edited rows: those that
        ask for a presence / frequency / repetition penalty, an allow-list or
        a logit bias.  Their logits are their own (``_row_logits``, a scratch
        entry of their own); ``ops.gemm.penalise`` edits them in place by each row's history
        (``hist`` int32 [slots][max_ctx], ``spans`` int32 [R][4], ``params``
        float32 [R][3]: ``csrc/kernels/penalty_kernels.h``).  Then a row with
        ``inv_temp > 0`` is drawn by ``ops.gemm.sample_truncated`` under its
        ``top_k`` / ``top_p`` (0 / 1.0: none) and a greedy row picked by
        ``ops.gemm.penalised_argmax``; the sampler never sees a greedy row
        (its contract wants ``inv_temp > 0``).  ``edit`` = (ids int32 [N],
        vals float32 [N], spans int32 [R][4]): the rows' allow lists and
        biases, applied by ``ops.gemm.logit_edit`` after the penalties
        (``csrc/kernels/logit_edit_kernels.h``); ``log_min_p`` float32 [R]:
        the sampling rows' min-p.  A row without a penalty has a span whose
        slot is -1 and reads no history; ``hist`` None: no row has one.
        ``n_greedy``: the rows come
        greedy first, so many of them (the engine lists them so).  Without
        it the rows are partitioned here, which reads ``inv_temp`` back on
        the host (a synchronisation)."""
        from . import gemm as G
        R, V = x.shape[0], w.shape[0]
        order = None
        if n_greedy is None:
            hot = inv_temp[:R] > 0
            n_greedy = R - int(hot.sum())
            if 0 < n_greedy < R:
                order = torch.argsort(hot.to(torch.uint8), stable=True)
                x, inv_temp, keys, top_k, top_p, spans, params = (
                    t[:R].index_select(0, order) for t in (x, inv_temp, keys, top_k, top_p, spans, params))
                if edit is not None:
                    edit = (edit[0], edit[1], edit[2][:R].index_select(0, order))
                if log_min_p is not None:
                    log_min_p = log_min_p[:R].index_select(0, order)
        lg = self._row_logits(x, w, "pen")
        if hist is not None:
            G.penalise(lg, hist, spans.contiguous(), params.contiguous(), vocab=V)
        if edit is not None:
            G.logit_edit(lg, edit[0].contiguous(), edit[1].contiguous(), edit[2].contiguous(), vocab=V)
        g = min(max(int(n_greedy), 0), R)
        out = torch.zeros(R, dtype=torch.int32, device=x.device)
        if g < R:
            G.sample_truncated(lg[g:], inv_temp.contiguous()[g:], keys.contiguous()[g:], top_k.contiguous()[g:],
                               top_p.contiguous()[g:], vocab=V, out=out[g:],
                               log_min_p=None if log_min_p is None else log_min_p.contiguous()[g:])
        if g:
            G.penalised_argmax(lg[:g], vocab=V, out=out)
        return out if order is None else torch.empty_like(out).index_copy_(0, order, out)

    def history_record(self, hist, tok, pos, slot, rows):
        """Record the token rows ``rows`` of a forward in the device-side
        token history (``ops.gemm.history_record``)."""
        from . import gemm as G
        G.history_record(hist, tok.contiguous(), pos.contiguous(), slot.contiguous(), rows.contiguous())

    def stop_match(self, tok, hist, rows, ent):
        """Per row the lowest stop entry that ends its generated tokens, the
        step's token ``tok`` (int32 [R]) included, or -1 -> int32 [R]
        (``ops.gemm.stop_match``; ``csrc/kernels/stop_kernels.h``)."""
        from . import gemm as G
        return G.stop_match(tok.to(torch.int32).contiguous(), hist, rows.contiguous(), ent.contiguous())

    def mlp_up(self, x: torch.Tensor, w_gu: torch.Tensor, fused: bool, min_fused_tokens: int) -> torch.Tensor:
        """silu(x·Wgᵀ) * (x·Wuᵀ).  ``fused``: ``w_gu`` is in swiglu order and
        steps of >= ``min_fused_tokens`` rows run the hand-written GEMM with
        the SwiGLU epilogue (one launch, no [T][2F] intermediate); smaller
        steps keep hipBLASLt + the permuted silu_mul."""
        if not fused:
            return self.silu_mul(torch.nn.functional.linear(x, w_gu))
        from . import gemm as G
        if x.shape[0] >= min_fused_tokens and G.supported(x.shape[0], w_gu.shape[0], x.shape[1]):
            return G.gemm_swiglu(x, w_gu)
        return self.silu_mul(torch.nn.functional.linear(x, w_gu), perm=True)

    def rope_kv(self, qkv, pos, slot, cos_t, sin_t, Hq, Hkv, kc, vc, q_out=None):
        _check(qkv, torch.bfloat16, "qkv")
        _check(pos, torch.int32, "pos")
        _check(slot, torch.int32, "slot")
        T = qkv.shape[0]
        if qkv.shape[1] != (Hq + 2 * Hkv) * 128:
            raise ValueError("qkv width mismatch")
        S, hk, max_ctx, hd = kc.shape
        if hk != Hkv or hd != 128 or vc.shape != kc.shape:
            raise ValueError("kv cache shape mismatch")
        q = q_out if q_out is not None else torch.empty((T, Hq * 128), dtype=qkv.dtype, device=qkv.device)
        self.k.rope_kv(qkv.data_ptr(), pos.data_ptr(), slot.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(), T,
                       Hq, Hkv, max_ctx, S, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), _stream(qkv))
        return q

    def _attn_args(self, q, kc, vc, Hq, Hkv, out):
        """Validate what both attention entry points hand to the kernels as
        raw pointers; returns the output tensor."""
        _check(q, torch.bfloat16, "q")
        if q.dim() != 2 or q.shape[1] != Hq * 128:
            raise ValueError("q must be [T, Hq * 128]")
        _check(kc, torch.bfloat16, "kc")
        _check(vc, torch.bfloat16, "vc")
        if kc.dim() != 4 or kc.shape[1] != Hkv or kc.shape[3] != 128 or vc.shape != kc.shape:
            raise ValueError("kv cache shape mismatch")
        if kc.device != q.device or vc.device != q.device:
            raise ValueError("kv cache must be on q's device")
        if out is None:
            return torch.empty_like(q)
        _check(out, torch.bfloat16, "out")
        if out.shape != q.shape or out.device != q.device:
            raise ValueError("out must match q's shape and device")
        return out

    def attention(self, q, kc, vc, pos, slot, Hq, Hkv, scale, out=None):
        o = self._attn_args(q, kc, vc, Hq, Hkv, out)
        _check(pos, torch.int32, "pos")
        _check(slot, torch.int32, "slot")
        T = q.shape[0]
        if pos.shape != (T,) or slot.shape != (T,):
            raise ValueError("pos and slot must be [T]")
        if pos.device != q.device or slot.device != q.device:
            raise ValueError("pos and slot must be on q's device")
        max_ctx = kc.shape[2]
        self.k.attention(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), pos.data_ptr(), slot.data_ptr(), T, Hq, Hkv,
                         max_ctx, kc.shape[0], float(scale), o.data_ptr(), _stream(q))
        return o

    MIXED_ATTENTION = os.environ.get("LLMQ_ATTN_MIXED", "1") != "0"

    def attention_tiles(self, q, kc, vc, tiles, Hq, Hkv, scale, out=None, n_dec: int = 0, seg_keys: int = 32,
                        mixed: bool = None):
        """Tiled attention; ``tiles`` int32 [n, 4] on the device = (first
        token row, n <= 16, slot, first position).  The first ``n_dec`` tiles
        must be 1-token (decode) tiles: they run on the wave-per-item decode
        kernel, the rest on the MFMA segment kernel (``seg_keys`` keys per
        block: 32 or 64).  ``mixed`` (default on; env LLMQ_ATTN_MIXED=0
        turns it off): a step with both kinds runs them in ONE launch."""
        o = self._attn_args(q, kc, vc, Hq, Hkv, out)
        if tiles.dtype != torch.int32 or tiles.dim() != 2 or tiles.shape[1] != 4 or not tiles.is_contiguous():
            raise ValueError("tiles must be a contiguous int32 [n, 4] tensor")
        if tiles.device != q.device:
            raise ValueError("tiles must be on q's device")
        self.k.attention_tiles(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), tiles.data_ptr(), tiles.shape[0],
                               int(n_dec), Hq, Hkv, kc.shape[2], kc.shape[0], q.shape[0], float(scale),
                               o.data_ptr(), _stream(q), int(seg_keys),
                               self.MIXED_ATTENTION if mixed is None else bool(mixed))
        return o


def make_tiles(seg_start, seg_len, seg_slot, seg_pos0, tile: int = 16):
    """Cut segments (runs of consecutive positions of one slot) into
    attention tiles of <= ``tile`` tokens: int32 [n, 4] numpy array."""
    out = []
    for st, n, sl, p0 in zip(seg_start, seg_len, seg_slot, seg_pos0):
        for a in range(0, n, tile):
            out.append((st + a, min(tile, n - a), sl, p0 + a))
    import numpy as _np
    return _np.asarray(out, dtype=_np.int32).reshape(-1, 4)


class RefOps:
    """fp32 PyTorch reference of the same math (bf16 in / bf16 out)."""

    def rmsnorm(self, x, w, eps, residual=None, out=None):
        xf = x.float()
        if residual is not None:
            r = (xf + residual.float()).to(torch.bfloat16)
            residual.copy_(r)
            xf = r.float()
        y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()
        y = y.to(torch.bfloat16)
        if out is not None:
            out.copy_(y)
            return out
        return y

    def silu_mul(self, gu, out=None, perm: bool = False):
        F = gu.shape[1] // 2
        if perm:
            from .gemm import swiglu_perm_index
            gu = gu.index_select(1, swiglu_perm_index(F, gu.device).argsort())
        g, u = gu[:, :F].float(), gu[:, F:].float()
        y = (torch.nn.functional.silu(g) * u).to(torch.bfloat16)
        if out is not None:
            out.copy_(y)
            return out
        return y

    def row_rms(self, x, eps):
        xf = x.float()
        return torch.rsqrt(xf.pow(2).mean(-1) + eps)

    def swiglu_rows(self, x, w_perm, r):
        """Reference of ``HipOps.swiglu_rows`` (fp32 math, one bf16 rounding)."""
        from .gemm import swiglu_unpermute
        w = swiglu_unpermute(w_perm).float()
        F = w.shape[0] // 2
        gu = (x.float() * r[:, None]) @ w.t()
        return (torch.nn.functional.silu(gu[:, :F]) * gu[:, F:]).to(torch.bfloat16)

    def qkv_rope_rows(self, x, wqkv, r, pos, slot, cos_t, sin_t, Hq, Hkv, kc, vc, split=True, split_full=None):
        qkv = ((x.float() * r[:, None]) @ wqkv.float().t()).to(torch.bfloat16)
        return self.rope_kv(qkv, pos, slot, cos_t, sin_t, Hq, Hkv, kc, vc)

    def greedy_head(self, x, w, fused: bool = True, min_rows: int = 256):
        return torch.argmax(torch.nn.functional.linear(x, w), dim=-1).to(torch.int32)

    def sample_head(self, x, w, inv_temp, keys, fused: bool = True, min_rows: int = 256):
        """Reference of ``HipOps.sample_head`` (the CPU path and the tests'
        oracle): fp32 logits, the numpy twin's noise, float64 scores."""
        from .sampling import sample_reference
        M = x.shape[0]
        lg = (x.float() @ w.float().t()).cpu().numpy()
        kk = self._keys(keys, M)
        it = inv_temp[:M]
        picks = torch.from_numpy(sample_reference(lg, it.cpu().numpy(), kk)).to(x.device)
        # a greedy row is exactly this class's greedy_head (bf16 logits)
        return torch.where(it != 0, picks, self.greedy_head(x, w, fused, min_rows))

    @staticmethod
    def _bf16_logits(x, w):
        """The rows' logits as ``HipOps._row_logits`` stores them: fp32
        products rounded to bf16 (a CPU tensor)."""
        return (x.float() @ w.float().t()).to(torch.bfloat16).cpu().contiguous()

    @staticmethod
    def _keys(keys, R):
        """The first ``R`` row keys as the numpy twins take them (uint32 [R][2])."""
        return keys[:R].cpu().contiguous().view(torch.int32).numpy().view("uint32")

    def truncated_head(self, x, w, inv_temp, keys, top_k, top_p, log_min_p=None):
        """Reference of ``HipOps.truncated_head``: fp32 logits rounded to bf16,
        then the numpy twin (``ops.sampling.sample_truncated_reference``)."""
        from .sampling import sample_truncated_reference
        R = x.shape[0]
        lg = self._bf16_logits(x, w).float().numpy()
        kk = self._keys(keys, R)
        picks = sample_truncated_reference(lg, inv_temp[:R].cpu().numpy(), kk, top_k[:R].cpu().numpy(),
                                           top_p[:R].cpu().numpy(),
                                           log_min_p=None if log_min_p is None else log_min_p[:R].cpu().numpy())
        return torch.from_numpy(picks).to(x.device)

    def logprob_head(self, x, w, tok):
        """Reference of ``HipOps.logprob_head``: fp32 logits rounded to bf16,
        then the numpy twin in float64 (``ops.sampling.logprob_reference``)."""
        from .sampling import logprob_reference
        lp, ids = logprob_reference(self._bf16_logits(x, w).float().numpy(), tok.cpu().numpy())
        return (torch.from_numpy(lp.astype("float32")).to(x.device),
                torch.from_numpy(ids.astype("int32")).to(x.device))

    def penalised_head(self, x, w, inv_temp, keys, top_k, top_p, hist, spans, params, n_greedy=None, edit=None,
                       log_min_p=None):
        """Reference of ``HipOps.penalised_head``: fp32 logits rounded to bf16,
        the numpy twins of the edits (``ops.sampling.penalise_rows_reference``,
        ``logit_edit_reference``),
        then ``sample_truncated_reference`` for a row with ``inv_temp > 0``
        and ``penalised_pick_reference`` for a greedy one."""
        from .sampling import (bf16_values, logit_edit_reference, penalise_rows_reference, penalised_pick_reference,
                               sample_truncated_reference)
        R, V = x.shape[0], w.shape[0]
        bits = self._bf16_logits(x, w).view(torch.int16).numpy().view("uint16")
        if hist is not None:
            bits = penalise_rows_reference(bits, V, hist.cpu().numpy(), spans[:R].cpu().numpy(),
                                           params[:R].cpu().numpy())
        if edit is not None:
            bits = logit_edit_reference(bits, V, edit[0].cpu().numpy(), edit[1].cpu().numpy(),
                                        edit[2][:R].cpu().numpy())
        it = inv_temp[:R].cpu().numpy()
        picks = penalised_pick_reference(bits, V)
        hot = it > 0
        if hot.any():
            picks[hot] = sample_truncated_reference(bf16_values(bits)[hot], it[hot], self._keys(keys, R)[hot],
                                                    top_k[:R].cpu().numpy()[hot], top_p[:R].cpu().numpy()[hot],
                                                    log_min_p=None if log_min_p is None
                                                    else log_min_p[:R].cpu().numpy()[hot])
        return torch.from_numpy(picks).to(x.device)

    def history_record(self, hist, tok, pos, slot, rows):
        """Reference of ``HipOps.history_record``."""
        r = rows.long()
        hist[slot.long()[r], pos.long()[r]] = tok[r].to(hist.dtype)

    def stop_match(self, tok, hist, rows, ent):
        """Reference of ``HipOps.stop_match``: the numpy twin."""
        from .sampling import stop_match_reference
        return torch.from_numpy(stop_match_reference(
            tok.cpu().numpy(), None if hist is None else hist.cpu().numpy(), rows.cpu().numpy(),
            ent.cpu().numpy())).to(tok.device)

    def mlp_up(self, x, w_gu, fused: bool, min_fused_tokens: int):
        """Reference of ``HipOps.mlp_up`` (``w_gu`` in swiglu order if fused)."""
        if fused:
            from .gemm import swiglu_unpermute
            w_gu = swiglu_unpermute(w_gu)
        return self.silu_mul(torch.nn.functional.linear(x, w_gu))

    def rope_kv(self, qkv, pos, slot, cos_t, sin_t, Hq, Hkv, kc, vc, q_out=None):
        T = qkv.shape[0]
        x = qkv.float().view(T, Hq + 2 * Hkv, 128)
        c = cos_t[pos.long()].unsqueeze(1)   # [T,1,64]
        s = sin_t[pos.long()].unsqueeze(1)

        def rot(v):
            a, b = v[..., :64], v[..., 64:]
            return torch.cat([a * c - b * s, b * c + a * s], dim=-1)

        q = rot(x[:, :Hq]).to(torch.bfloat16).reshape(T, Hq * 128)
        k = rot(x[:, Hq:Hq + Hkv]).to(torch.bfloat16)
        v = x[:, Hq + Hkv:].to(torch.bfloat16)
        for t in range(T):
            kc[slot[t], :, pos[t]] = k[t]
            vc[slot[t], :, pos[t]] = v[t]
        if q_out is not None:
            q_out.copy_(q)
            return q_out
        return q

    def attention(self, q, kc, vc, pos, slot, Hq, Hkv, scale, out=None):
        T = q.shape[0]
        G = Hq // Hkv
        res = torch.empty_like(q)
        qf = q.float().view(T, Hq, 128)
        for t in range(T):
            n = int(pos[t]) + 1
            K = kc[slot[t], :, :n].float()       # [Hkv, n, 128]
            V = vc[slot[t], :, :n].float()
            Kx = K.repeat_interleave(G, dim=0)   # [Hq, n, 128]
            Vx = V.repeat_interleave(G, dim=0)
            sc = torch.einsum("hd,hnd->hn", qf[t], Kx) * scale
            p = torch.softmax(sc, dim=-1)
            res[t] = torch.einsum("hn,hnd->hd", p, Vx).reshape(-1).to(torch.bfloat16)
        if out is not None:
            out.copy_(res)
            return out
        return res

    def attention_tiles(self, q, kc, vc, tiles, Hq, Hkv, scale, out=None, n_dec: int = 0, seg_keys: int = 32):
        """Reference: expand tiles to per-token (pos, slot) and reuse ``attention``."""
        t = tiles.cpu().long()
        T = q.shape[0]
        pos = torch.zeros(T, dtype=torch.long)
        slot = torch.zeros(T, dtype=torch.long)
        for r0, n, sl, p0 in t.tolist():
            pos[r0:r0 + n] = torch.arange(p0, p0 + n)
            slot[r0:r0 + n] = sl
        return self.attention(q, kc, vc, pos, slot, Hq, Hkv, scale, out=out)


def rope_tables(max_pos: int, theta: float = 500000.0, device="cpu"):
    inv = 1.0 / (theta ** (torch.arange(0, 64, dtype=torch.float64) / 64.0))
    t = torch.arange(max_pos, dtype=torch.float64)
    f = torch.outer(t, inv)
    return f.cos().float().to(device).contiguous(), f.sin().float().to(device).contiguous()


def get_ops(impl: str):
    if impl == "hip":
        return HipOps()
    if impl == "ref":
        return RefOps()
    raise ValueError(f"unknown op implementation {impl!r}")
