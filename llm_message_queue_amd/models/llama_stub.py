"""Llama-3-8B-shaped backend stub (N12): random-init bf16 weights, one
instance per GPU, serving the gateway's dispatched requests.

The reference never calls its endpoints (`internal/loadbalancer/load_balancer.go:35-49`,
URLs from `internal/scheduler/scheduler.go:299-301`); here each endpoint is a
real GPU worker so load signals (in-flight slots, HBM) are live.

Forward = one continuous-batching step over T tokens (chunked-prefill and
decode tokens mixed).  GEMMs: ``torch.nn.functional.linear`` (hipBLASLt).
The o / down projections accumulate into the residual stream in the GEMM
epilogue (beta = 1).  Everything else: hand-written HIP kernels
(``ops.llama_ops.HipOps``): RMSNorm (optionally fused with the residual add), RoPE + KV-cache write, segment-tiled MFMA GQA attention
over the slot KV cache (prefill chunks and decode tokens), SiLU*up -- and,
with ``fused_mlp`` (default with the HIP ops), the hand-written gfx950 GEMM
with the SwiGLU epilogue for the gate/up projection (``ops.gemm``): the
[T][2F] gate/up product never reaches HBM and the silu_mul pass disappears
(``profiles/r2_gemm_swiglu.md``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from ..ops import gemm as G
from ..ops import quant as Qn
from ..ops.llama_ops import get_ops, rope_tables
from . import routes as R


@dataclass
class LlamaConfig:
    vocab: int = 128256
    dim: int = 4096
    layers: int = 32
    heads: int = 32
    kv_heads: int = 8
    head_dim: int = 128
    ffn: int = 14336
    rope_theta: float = 500000.0
    eps: float = 1e-5

    @classmethod
    def llama3_8b(cls) -> "LlamaConfig":
        return cls()

    @classmethod
    def tiny(cls) -> "LlamaConfig":
        """Smoke/CPU-test size (same kernels, same head_dim=128, GQA 4)."""
        return cls(vocab=1024, dim=2048, layers=2, heads=16, kv_heads=4, ffn=2048)

    @classmethod
    def by_name(cls, name: str) -> "LlamaConfig":
        n = name.lower().replace("_", "-")
        if n in ("llama3-8b", "llama-3-8b", "llama3_8b", "8b"):
            return cls.llama3_8b()
        if n == "tiny":
            return cls.tiny()
        raise ValueError(f"unknown backend model {name!r}")

    def param_count(self) -> int:
        d, f = self.dim, self.ffn
        qkv = d * (self.heads + 2 * self.kv_heads) * self.head_dim
        per = qkv + d * d + 2 * d * f + d * f + 2 * d
        return self.layers * per + 2 * self.vocab * d + d

    def quant_bytes(self) -> int:
        """Bytes of the layers' FP8 copy (``small_weights="fp8"``): a byte
        an element of the four layer matrices + a float32 scale a row."""
        d, f = self.dim, self.ffn
        nqkv = (self.heads + 2 * self.kv_heads) * self.head_dim
        return self.layers * (nqkv * d + d * d + 3 * d * f + 4 * (nqkv + d + 2 * f + d))


# the layer weights a ``quant`` forward reads as FP8 (e4m3 codes + a scale a row)
QUANT_NAMES = ("wqkv", "wo", "w_gu", "w_down")
QUANT_NAMES_BY_MODE = {"bf16": (), "fp8": QUANT_NAMES}


def _given(**kw) -> dict:
    """The keyword arguments that are set: a head is passed an optional input
    only where a row of the step uses it, so a step without one makes the
    call it made before the option existed."""
    return {k: v for k, v in kw.items() if v is not None}


class Truncate(NamedTuple):
    """``forward(trunc=...)``: the sampled rows that ask for top-k / top-p /
    min-p and are drawn again, from their own logits, by
    ``ops.truncated_head`` (the head over all sampled rows runs as without
    it; their first draw is overwritten)."""
    rows: torch.Tensor                        # int64 [R] into the sampled rows
    top_k: torch.Tensor                       # int32 [R] (0: none)
    top_p: torch.Tensor                       # float32 [R] (1.0: none)
    log_min_p: Optional[torch.Tensor] = None  # float32 [R] (``ops.sampling.min_p_log``; -inf: off) or None


class LogitEdit(NamedTuple):
    """The allow lists and logit biases of a step's edited rows
    (``ops.gemm.logit_edit``)."""
    ids: torch.Tensor                         # int32 [N]: the rows' lists, packed
    vals: torch.Tensor                        # float32 [N]
    spans: torch.Tensor                       # int32 [P][4]: (allow_off, n_allow, bias_off, n_bias) per row


class Penalise(NamedTuple):
    """``forward(pen=...)``: the device-side token history, the token rows of
    this forward to record in it, and the sampled rows that ask for a
    presence / frequency / repetition penalty, an allow-list or a logit bias,
    greedy or sampling.  Those rows are drawn again by ``ops.penalised_head``
    with their own ``top_k`` / ``top_p`` / ``log_min_p`` and overwrite their
    first draw; the caller keeps them out of ``trunc``, so a row is drawn
    again once.  A row with only an allow-list or a bias has a penalty span
    whose slot is -1."""
    hist: Optional[torch.Tensor]              # int32 [slots][max_ctx]; None where no slot has a penalty
    #                                           (nothing is recorded or read then)
    record: Optional[torch.Tensor]            # int32 [Q]: token rows of this forward to record in ``hist``
    rows: torch.Tensor                        # int64 [P] into the sampled rows, the greedy ones first
    spans: torch.Tensor                       # int32 [P][4]: (slot, from, split, end) in ``hist``
    params: torch.Tensor                      # float32 [P][3]: presence, frequency, repetition
    top_k: torch.Tensor                       # int32 [P]
    top_p: torch.Tensor                       # float32 [P]
    n_greedy: Optional[int]                   # so many of ``rows`` are greedy
    edit: Optional[LogitEdit] = None
    log_min_p: Optional[torch.Tensor] = None  # float32 [P] or None


class Stops(NamedTuple):
    """``forward(stop=...)``: the sampled rows that have stop tokens or stop
    sequences (``csrc/kernels/stop_kernels.h``).  After the last overwrite
    of the tokens ``ops.stop_match`` compares each such row's generated
    tokens with its entries."""
    hist: Optional[torch.Tensor]              # int32 [slots][max_ctx] or None (no entry longer than one token)
    record: Optional[torch.Tensor]            # int32 [Q] token rows to record in ``hist`` where ``pen`` does not
    #                                           already (the engine merges them into ``pen``'s list), or None
    rows: torch.Tensor                        # int64 [R] into the sampled rows
    records: torch.Tensor                     # int32 [R][6]: (slot, gen_from, end, min_tokens, ent_off, n_ent)
    entries: torch.Tensor                     # int32 [N][9]: length, then up to 8 token ids


class HeadOut(NamedTuple):
    """What ``forward`` returns when ``logp`` or ``stop`` is given; the
    fields not asked for are None."""
    tokens: torch.Tensor                      # int32 [S]
    lp: Optional[torch.Tensor]                # float32 [L][6]: the chosen token's score, then the 5 most likely
    ids: Optional[torch.Tensor]               # int32 [L][5]
    stop_flags: Optional[torch.Tensor]        # int32 [R]: the matched entry, -1: none


class LlamaStub:
    def __init__(self, cfg: LlamaConfig, slots: int, max_ctx: int, device="cuda", impl: str = "hip",
                 seed: int = 0, dtype=torch.bfloat16, residual_in_gemm: bool = True, split_qkv: bool = False,
                 fused_mlp: Optional[bool] = None, min_fused_tokens: int = 512,
                 fused_qkv: Optional[bool] = None, min_fused_qkv_tokens: int = 2048, row_scale_norm: bool = True,
                 fused_head: Optional[bool] = None, fused_resid: Optional[bool] = None,
                 fused_rms: Optional[bool] = None,
                 prune_last: bool = True, library_gemm: bool = False, small_weights: str = "bf16"):
        if cfg.head_dim != 128:
            raise ValueError("kernels assume head_dim = 128")
        if small_weights not in QUANT_NAMES_BY_MODE:
            raise ValueError(f"small_weights must be bf16 / fp8, not {small_weights!r}")
        self.cfg = cfg
        self.device = torch.device(device)
        self.ops = get_ops(impl)
        self.impl = impl
        self.slots = slots
        self.max_ctx = max_ctx
        # o / down projections accumulate straight into the residual stream
        # (hipBLASLt beta = 1: res += a @ W^T, one rounding); the following
        # RMSNorm then only reads res -- half its HBM traffic
        # (profiles/r1_gemm_experiments.md).  False: F.linear + fused
        # residual-add RMSNorm.
        self.residual_in_gemm = residual_in_gemm
        # the last layer's o projection and MLP only for the step's sampled
        # rows (see ``hidden``); False: every row, then select (A/B)
        self.prune_last = bool(prune_last)
        # QKV as two GEMMs (q: d x d, kv: 2*kv_heads*hd x d) written into
        # column slices of one qkv buffer: the fused 6144-wide GEMM at
        # T = 4096 is 384 256x256 tiles = 1.5 rounds over 256 CUs; the split
        # pair measured ~15% faster in isolation (bench/qkv_split.py) and cut
        # in-model GEMM time 4.3%, but the serving step did not get shorter
        # (profiles/r1_gemm_experiments.md), so it is off by default.  The
        # weight stays one tensor; its row slices are contiguous views.
        self.split_qkv = split_qkv
        # gate/up weight kept in the fused kernel's swiglu row order (same
        # random draw, rows permuted once at init) so the HIP path runs
        # gemm_swiglu on steps of >= min_fused_tokens rows
        self.fused_mlp = (impl == "hip") if fused_mlp is None else bool(fused_mlp)
        self.min_fused_tokens = int(min_fused_tokens)
        # qkv projection with the RoPE + K/V-cache-write epilogue (ops.gemm.qkv_rope)
        # on steps of >= min_fused_qkv_tokens rows (3.5% faster than hipBLASLt +
        # rope_kv at T = 4041, slower below ~2k rows: profiles/r2_gemm_swiglu.md)
        self.fused_qkv = (impl == "hip" and not split_qkv) if fused_qkv is None else bool(fused_qkv)
        self.min_fused_qkv_tokens = int(min_fused_qkv_tokens)
        # LM head + greedy argmax in one hand-written GEMM (argmax epilogue, no
        # [rows][vocab] logits) when the step samples >= 256 rows
        self.fused_head = (impl == "hip") if fused_head is None else bool(fused_head)
        # o / down projections into the residual on the hand-written kernel
        # (ops.gemm.RESID_EPI: the residual tile staged into LDS by DMA and
        # added in place) when its 256x256 tiles fill whole waves of the chip
        # (the saturated serving step: T ~ 4,040 -> 256 tiles); hipBLASLt's
        # beta = 1 stream-K kernel otherwise (ops.gemm.residual_tiles_ok).
        # Default since round 5: faster than hipBLASLt in isolation (o 94.8 vs
        # 95.3 us, down 299.7 vs 304.3 us at T = 4041,
        # profiles/r5_resid_ab_1gpu.jsonl) and >= it in the serving A/B
        # (profiles/r5_resid_serving_ab_1gpu.jsonl).
        self.fused_resid = (impl == "hip") if fused_resid is None else bool(fused_resid)
        # with the residual GEMM: the RMSNorm row scales of the updated
        # residual rows out of its epilogue (ops.gemm.gemm_residual_rms)
        # instead of a separate row_rms pass.  Off by default: the epilogue's
        # cross-block reduction adds 0.5-7 us to the tail of a single-wave
        # GEMM, more than the 12.8 us row_rms launch it removes saves
        # (profiles/r5_resid_rms_bench.jsonl, profiles/r5_fused_rms_serving_ab_1gpu.jsonl)
        self.fused_rms = False if fused_rms is None else bool(fused_rms)
        # False (the default since round 6): no library GEMM at any row
        # count -- skinny for small steps, 256x256 tiles (split-K where whole
        # tiles leave CUs idle) above, the argmax head at any row count.
        # True: hipBLASLt where it was faster (sub-wave o / down, the head
        # under 256 rows); measured equal within 0.4 % on the bench
        # (profiles/r6_realtime_modes.md).  fused_resid=False keeps the library.
        self.library_gemm = bool(library_gemm) or impl != "hip" or not self.fused_resid
        self._cus = G._cu_count(self.device) if (self.fused_resid and self.device.type == "cuda") else 0
        # fused paths take the raw residual rows + a per-row RMSNorm scale
        # (True) or an rmsnorm'd copy of the rows (False, A/B)
        self.row_scale_norm = bool(row_scale_norm)
        # "fp8": every layer also holds its four weight matrices as e4m3
        # codes + one power-of-two scale a row (ops.quant), which a forward
        # with ``quant`` reads instead of the bf16 ones (W8A16: half the
        # bytes a small step streams; ops.gemm.skinny_fp8).  The embedding
        # and the LM head stay bf16.
        self.small_weights = small_weights
        if small_weights == "fp8" and impl == "hip" and not (
                self.fused_mlp and self.fused_qkv and self.row_scale_norm and self.residual_in_gemm):
            raise ValueError("small_weights fp8 needs the fused paths (fused_mlp, fused_qkv, row_scale_norm, "
                             "residual_in_gemm)")
        self.route_flags = self._route_flags()
        g = torch.Generator(device=self.device).manual_seed(seed)
        std = 0.02

        def w(*shape):
            return (torch.randn(*shape, generator=g, device=self.device, dtype=torch.float32) * std).to(dtype)

        d, hq, hkv, hd = cfg.dim, cfg.heads, cfg.kv_heads, cfg.head_dim
        self.embed = w(cfg.vocab, d)
        self.lm_head = w(cfg.vocab, d)
        self.final_norm = torch.ones(d, dtype=dtype, device=self.device)
        self.layers = []
        for _ in range(cfg.layers):
            L = {
                "attn_norm": torch.ones(d, dtype=dtype, device=self.device),
                "wqkv": w((hq + 2 * hkv) * hd, d),
                "wo": w(d, hq * hd),
                "mlp_norm": torch.ones(d, dtype=dtype, device=self.device),
                "w_gu": w(2 * cfg.ffn, d),
                "w_down": w(d, cfg.ffn),
            }
            # the fused paths read the raw residual rows: the RMSNorm weight
            # moves into the projection's input columns (W' = W diag(g)) and
            # the norm left on the small-step path becomes a unit-weight one
            if self.fused_qkv:
                L["wqkv"], L["attn_norm"] = self._fold_norm(L["wqkv"], L["attn_norm"])
            if self.fused_mlp:
                L["w_gu"], L["mlp_norm"] = self._fold_norm(L["w_gu"], L["mlp_norm"])
            L["w_gu"] = self._gu_layout(L["w_gu"])
            if small_weights == "fp8":
                L["fp8"] = {k: self._quantize(L[k]) for k in QUANT_NAMES}
            self.layers.append(L)
        # KV cache: per layer [slots, kv_heads, max_ctx, head_dim]
        self.kcache = [torch.zeros((slots, hkv, max_ctx, hd), dtype=dtype, device=self.device)
                       for _ in range(cfg.layers)]
        self.vcache = [torch.zeros((slots, hkv, max_ctx, hd), dtype=dtype, device=self.device)
                       for _ in range(cfg.layers)]
        self.cos, self.sin = rope_tables(max_ctx, cfg.rope_theta, self.device)
        self.scale = 1.0 / math.sqrt(hd)

    def _route_flags(self) -> R.RouteFlags:
        """What ``models.routes`` plans from, read once when the model is built."""
        cfg = self.cfg
        return R.RouteFlags(
            hip=self.impl == "hip", residual_in_gemm=bool(self.residual_in_gemm), split_qkv=bool(self.split_qkv),
            fused_mlp=self.fused_mlp, fused_qkv=self.fused_qkv, row_scale_norm=self.row_scale_norm,
            fused_rms=self.fused_rms, prune_last=self.prune_last, library_gemm=self.library_gemm,
            min_fused_tokens=self.min_fused_tokens, min_fused_qkv_tokens=self.min_fused_qkv_tokens, cus=self._cus,
            dim=cfg.dim, n_qkv=(cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim)

    @staticmethod
    def _fold_norm(w: torch.Tensor, g: torch.Tensor):
        if not bool((g == 1).all()):
            w = (w.float() * g.float()[None, :]).to(w.dtype)
        return w, torch.ones_like(g)

    def _gu_layout(self, w_gu: torch.Tensor) -> torch.Tensor:
        if not self.fused_mlp:
            return w_gu
        return G.swiglu_permute(w_gu)

    def _quantize(self, w: torch.Tensor):
        """(codes, scale) of one layer weight, on the device kernel with the
        HIP ops (bit-equal to the host twin)."""
        if self.impl == "hip" and w.is_cuda:
            return G.quantize_rows(w)
        codes, scale = Qn.quantize_rows_e4m3(w)
        return codes.to(w.device), scale.to(w.device)

    def _dequantized(self, i: int) -> dict:
        """Layer ``i`` with its quantised weights decoded back to bf16: what
        the reference ops compute a ``quant`` forward with (a cache of the
        reference path only; the HIP path reads the codes)."""
        cache = self.__dict__.setdefault("_deq_layers", {})
        if i not in cache:
            L = dict(self.layers[i])
            for k, (codes, scale) in L.pop("fp8").items():
                L[k] = Qn.dequantize(codes, scale)
            cache[i] = L
        return cache[i]

    def weight_bytes(self) -> int:
        n = self.embed.numel() + self.lm_head.numel() + self.final_norm.numel()
        q = 0
        for L in self.layers:
            n += sum(t.numel() for t in L.values() if torch.is_tensor(t))
            q += sum(c.numel() + 4 * s.numel() for c, s in L.get("fp8", {}).values())
        return n * 2 + q

    def kv_bytes(self) -> int:
        return sum(t.numel() * 2 for t in self.kcache) * 2

    @torch.no_grad()
    def forward(self, tokens: torch.Tensor, pos: torch.Tensor, slot: torch.Tensor,
                sample_idx: torch.Tensor, tiles: Optional[torch.Tensor] = None, n_dec: int = 0,
                small_cus: int = 0, inv_temp: Optional[torch.Tensor] = None,
                keys: Optional[torch.Tensor] = None, quant: bool = False, trunc=None, logp=None, pen=None,
                stop=None):
        """One step over T tokens; returns the next-token ids (int32) of the
        rows in ``sample_idx`` (the last token of each request's chunk).  In
        this order:
          1. the token rows ``pen.record`` / ``stop.record`` name are recorded
             in the device history (``ops.history_record``), before anything
             reads it; a forward that samples nothing still records;
          2. the trunk (``hidden``);
          3. the head over all sampled rows: with ``inv_temp`` (float32, 1 / T
             per sampled row, 0 = greedy) and ``keys`` (``ops.sampling.
             row_keys``) ``ops.sample_head`` (temperature sampling by
             Gumbel-max), else ``ops.greedy_head``;
          4. ``trunc`` (``Truncate``): its rows are drawn again, from their own
             logits, and overwrite their first draw;
          5. ``pen`` (``Penalise``): likewise, greedy or sampling;
          6. ``stop`` (``Stops``): ``ops.stop_match`` over the tokens as they
             now are.  No token is changed by it;
          7. ``logp`` (int64 [L] rows into the sampled rows, sampling or
             greedy): ``ops.logprob_head``'s scores of the tokens finally
             chosen (the tokens themselves are what they are without it).
        Returns the token tensor when neither ``logp`` nor ``stop`` is given,
        else a ``HeadOut``.
        ``tiles`` (int32 [n, 4], see ``ops.llama_ops.make_tiles``) groups the
        tokens into per-slot segments for the MFMA attention kernel (its first
        ``n_dec`` rows are 1-token decode tiles); without it attention runs
        per token.  ``small_cus`` > 0: a small step confined to that many CUs
        (a realtime micro-forward on its CU partition) -- every GEMM on the
        hand-written kernels whatever the row count (no library kernel, none
        of whose persistent / stream-K grids assume the whole chip), split-K
        where the tiles cannot fill the partition.  ``quant`` (a model built
        with ``small_weights="fp8"``): every layer GEMM of this forward reads
        the FP8 weights (``hidden``); the head stays bf16."""
        for opt in (pen, stop):
            if opt is not None and opt.hist is not None and opt.record is not None and opt.record.numel():
                self.ops.history_record(opt.hist, tokens, pos, slot, opt.record)
        step = R.plan_step(self.route_flags, small_cus)
        if step.prune:
            sel = self.hidden(tokens, pos, slot, tiles=tiles, n_dec=n_dec, rows=sample_idx, small_cus=small_cus,
                              quant=quant)
        else:
            sel = self.hidden(tokens, pos, slot, tiles=tiles, n_dec=n_dec,
                              small_cus=small_cus, quant=quant).index_select(0, sample_idx)
        sampling = inv_temp is not None and keys is not None
        if sampling:
            out = self.ops.sample_head(sel, self.lm_head, inv_temp, keys, self.fused_head,
                                       min_rows=step.head_min_rows)
            if trunc is not None:
                out.index_copy_(0, trunc.rows, self.ops.truncated_head(
                    sel.index_select(0, trunc.rows), self.lm_head, inv_temp.index_select(0, trunc.rows),
                    keys.index_select(0, trunc.rows), trunc.top_k, trunc.top_p, **_given(log_min_p=trunc.log_min_p)))
        else:
            out = self.ops.greedy_head(sel, self.lm_head, self.fused_head, min_rows=step.head_min_rows)
        if pen is not None and pen.rows.numel():
            P = pen.rows.numel()
            if sampling:
                it, kk = inv_temp.index_select(0, pen.rows), keys.index_select(0, pen.rows)
            else:                                     # an all-greedy step: no noise is read
                it = torch.zeros(P, dtype=torch.float32, device=out.device)
                kk = torch.zeros((P, 2), dtype=torch.int32, device=out.device)
            out.index_copy_(0, pen.rows, self.ops.penalised_head(
                sel.index_select(0, pen.rows), self.lm_head, it, kk, pen.top_k, pen.top_p, pen.hist, pen.spans,
                pen.params, n_greedy=pen.n_greedy, **_given(edit=pen.edit, log_min_p=pen.log_min_p)))
        if logp is None and stop is None:
            return out
        flags = lp = ids = None
        if stop is not None:
            flags = self.ops.stop_match(out.index_select(0, stop.rows), stop.hist, stop.records, stop.entries)
        if logp is not None:
            lp, ids = self.ops.logprob_head(sel.index_select(0, logp), self.lm_head, out.index_select(0, logp))
        return HeadOut(out, lp, ids, flags)

    @torch.no_grad()
    def hidden(self, tokens: torch.Tensor, pos: torch.Tensor, slot: torch.Tensor,
               tiles: Optional[torch.Tensor] = None, n_dec: int = 0,
               rows: Optional[torch.Tensor] = None, small_cus: int = 0, quant: bool = False) -> torch.Tensor:
        """The 32-layer trunk: final-normed hidden states [T, d] (writes the
        step's K/V into the cache).

        The residual stream ``res`` is updated in place by the o / down GEMMs.
        On steps large enough for the hand-written GEMMs, the RMSNorms before
        the qkv and gate/up projections are never materialised: ``row_rms``
        computes each row's scale, the norm weight is folded into W at init,
        and the GEMM epilogue applies the scale to its accumulator rows.
        Which kernel each GEMM takes is planned by ``models.routes``, three
        plans a step: the qkv projection, a layer's o + MLP block at the
        step's rows, and the last layer's block at the rows it keeps.

        ``rows`` (the step's sampled rows): the last layer writes every
        token's K/V and attends for every token as usual, then keeps only
        these rows for its o projection and MLP -- the other rows' outputs of
        that layer feed nothing (no later layer reads them, and the LM head
        reads only the sampled rows), so the result for ``rows`` is the same
        computation.  Returns [len(rows), d] then, else [T, d].

        ``quant``: the four GEMMs of every layer read the layer's FP8 weights
        -- with the HIP ops on ``ops.gemm.skinny_fp8`` or, from the row
        counts of ``ops.gemm.fp8_plan`` on, the FP8-weight tile kernel
        (``gemm_fp8`` / ``gemm_swiglu_fp8`` / ``gemm_residual_fp8``), up to
        ``SKINNY_CHUNKED_MAX_M`` rows (never a bf16 kernel: a request sees one
        model in all its forwards), with the reference ops on the decoded
        weights (``ops.quant.dequantize``), which is the same arithmetic."""
        cfg, ops = self.cfg, self.ops
        if quant and self.small_weights != "fp8":
            raise ValueError("quant forward on a model built without small_weights='fp8'")
        layers = self.layers
        if quant and self.impl != "hip":
            layers, quant = [self._dequantized(i) for i in range(len(self.layers))], False
        f = self.route_flags
        if R.plan_step(f, small_cus).residual_norm:
            return self._hidden_residual_norm(tokens, pos, slot, tiles, n_dec, layers)
        res = F.embedding(tokens, self.embed)            # [T, d], updated in place
        T = res.shape[0]
        if rows is not None and rows.numel() == T:
            rows = None                                  # every row sampled: nothing to drop
        qkv = R.plan_qkv(f, T, small_cus, quant)         # (refuses a quant step the fp8 kernel cannot take)
        block = R.plan_block(f, T, small_cus, quant)
        tail = R.plan_block(f, T if rows is None else rows.numel(), small_cus, quant, last=True)
        last = len(layers) - 1

        scale = None                                     # row scales of res from the previous down GEMM
        for i, L in enumerate(layers):
            a = self._attend(self._qkv_proj(qkv, res, scale, L, i, pos, slot), i, pos, slot, tiles, n_dec)
            if i == last and rows is not None:
                if rows.numel() == 0:                    # nothing sampled (a step of unfinished prefill
                    return res[:0]                       # chunks): K/V written, no row kernel gets 0 rows
                res, a = res.index_select(0, rows), a.index_select(0, rows)
            scale = self._mlp_block(res, a, L, tail if i == last else block)
        return ops.rmsnorm(res, self.final_norm, cfg.eps)

    @torch.no_grad()
    def warm_tail(self, sizes) -> int:
        """Run the last layer's o + MLP block (``_mlp_block``) once per row
        count in ``sizes`` on scratch rows: with ``prune_last`` that block
        sees the step's sampled-row count, not its token count, so its GEMM
        shapes get their own warm-up (a first use of a library kernel loads
        its code object)."""
        cfg = self.cfg
        L = self.layers[-1]
        n = 0
        for M in sizes:
            M = int(M)
            res = torch.zeros((M, cfg.dim), dtype=self.embed.dtype, device=self.device)
            a = torch.zeros((M, cfg.heads * cfg.head_dim), dtype=self.embed.dtype, device=self.device)
            self._mlp_block(res, a, L, R.plan_block(self.route_flags, M, 0, False, last=True))
            n += 1
        return n

    def _row_scale(self, p: R.Gemm, res: torch.Tensor, carried):
        """The RMSNorm row scales of ``res`` for GEMM ``p``: the ones the GEMM
        before it made in its epilogue, where there are any and ``p`` takes
        them, else a ``row_rms`` pass."""
        return carried if p.takes_scale and carried is not None else self.ops.row_rms(res, self.cfg.eps)

    def _qkv_proj(self, p: R.Gemm, res, scale, L, i, pos, slot):
        """Layer ``i``'s rotated q of the rows ``res`` (K/V written into the
        cache) on the kernel ``p`` names; ``scale``: the row scales the
        previous layer's down GEMM made, or None."""
        cfg, ops = self.cfg, self.ops
        kv = (pos, slot, self.cos, self.sin, cfg.heads, cfg.kv_heads, self.kcache[i], self.vcache[i])
        if p.kind == "tile_rows":
            return ops.qkv_rope_rows(res, L["wqkv"], self._row_scale(p, res, scale), *kv, split_full=p.split_full)
        if p.kind == "tile_normed":
            return G.qkv_rope(ops.rmsnorm(res, L["attn_norm"], cfg.eps), L["wqkv"], *kv)
        if p.kind == "library":
            return self._qkv(ops.rmsnorm(res, L["attn_norm"], cfg.eps), L, i, pos, slot)
        qkv = torch.empty((res.shape[0], L["wqkv"].shape[0]), dtype=res.dtype, device=res.device)
        rs = self._row_scale(p, res, scale)
        if p.kind == "tile_fp8":
            G.gemm_fp8(res, *L["fp8"]["wqkv"], out=qkv, row_scale=rs, split_cus=p.split_cus)
        elif p.kind == "skinny_fp8":
            G.skinny_fp8(res, *L["fp8"]["wqkv"], qkv, G.SK_STORE, row_scale=rs, cus=p.cus)
        elif p.kind == "skinny":
            G.skinny(res, L["wqkv"], qkv, G.SK_STORE, row_scale=rs, cus=p.cus)
        else:
            raise ValueError(f"no qkv kernel of kind {p.kind!r}")
        return ops.rope_kv(qkv, *kv)

    def _into_res(self, p: R.Gemm, x, L, name: str, res):
        """res += x . L[name]^T in place on the kernel ``p`` names; returns
        the RMSNorm row scales of the updated ``res`` where ``p`` makes them,
        else None."""
        if p.kind == "tile_rms":
            return G.gemm_residual_rms(x, L[name], res, self.cfg.eps)
        if p.kind == "skinny":
            G.skinny(x, L[name], res, G.SK_RESID, cus=p.cus)
        elif p.kind == "tile":
            G.gemm_residual(x, L[name], res, split_cus=p.split_cus)
        elif p.kind == "library":
            res.addmm_(x, L[name].t())
        elif p.kind == "tile_fp8":
            G.gemm_residual_fp8(x, *L["fp8"][name], res, split_cus=p.split_cus)
        elif p.kind == "skinny_fp8":
            G.skinny_fp8(x, *L["fp8"][name], res, G.SK_RESID, cus=p.cus)
        else:
            raise ValueError(f"no o / down kernel of kind {p.kind!r}")
        return None

    def _mlp_block(self, res: torch.Tensor, a: torch.Tensor, L: dict, plan: R.Block):
        """res += o(a); res += down(swiglu(norm(res))) -- in place, each GEMM
        on the kernel ``plan`` (``routes.plan_block`` for this block's row
        count) names.  Returns the RMSNorm row scales of the final ``res``
        where the down GEMM made them in its epilogue, else None."""
        cfg, ops = self.cfg, self.ops
        scale = self._into_res(plan.o, a, L, "wo", res)
        p, w = plan.gu, L["w_gu"]
        if p.kind in ("skinny", "skinny_fp8", "tile_fp8"):
            act = torch.empty((res.shape[0], w.shape[0] // 2), dtype=res.dtype, device=res.device)
            rs = self._row_scale(p, res, scale)
            if p.kind == "tile_fp8":
                G.gemm_swiglu_fp8(res, *L["fp8"]["w_gu"], out=act, row_scale=rs, split_cus=p.split_cus)
            elif p.kind == "skinny_fp8":
                G.skinny_fp8(res, *L["fp8"]["w_gu"], act, G.SK_SWIGLU, row_scale=rs, cus=p.cus)
            else:
                G.skinny(res, w, act, G.SK_SWIGLU, row_scale=rs, cus=p.cus)
        elif p.kind == "tile_split":
            act = G.gemm_swiglu(res, w, row_scale=self._row_scale(p, res, scale), split_cus=p.split_cus)
        elif p.kind == "rows":
            act = ops.swiglu_rows(res, w, self._row_scale(p, res, scale))
        elif p.kind == "tile_normed":
            act = G.gemm_swiglu(ops.rmsnorm(res, L["mlp_norm"], cfg.eps), w)
        elif p.kind == "mlp_up":
            act = ops.mlp_up(ops.rmsnorm(res, L["mlp_norm"], cfg.eps), w, self.fused_mlp, self.min_fused_tokens)
        else:
            raise ValueError(f"no gate/up kernel of kind {p.kind!r}")
        return self._into_res(plan.down, act, L, "w_down", res)

    def _qkv(self, x, L, i, pos, slot):
        """qkv projection (hipBLASLt) + RoPE / KV-cache write of normalised rows."""
        cfg, ops = self.cfg, self.ops
        if self.split_qkv:
            nq = cfg.heads * cfg.head_dim
            qkv = torch.empty((x.shape[0], L["wqkv"].shape[0]), dtype=x.dtype, device=x.device)
            torch.mm(x, L["wqkv"][:nq].t(), out=qkv[:, :nq])
            torch.mm(x, L["wqkv"][nq:].t(), out=qkv[:, nq:])
        else:
            qkv = F.linear(x, L["wqkv"])
        return ops.rope_kv(qkv, pos, slot, self.cos, self.sin, cfg.heads, cfg.kv_heads,
                           self.kcache[i], self.vcache[i])

    def _attend(self, q, i, pos, slot, tiles, n_dec):
        cfg, ops = self.cfg, self.ops
        if tiles is not None:
            return ops.attention_tiles(q, self.kcache[i], self.vcache[i], tiles, cfg.heads, cfg.kv_heads,
                                       self.scale, n_dec=n_dec)
        return ops.attention(q, self.kcache[i], self.vcache[i], pos, slot, cfg.heads, cfg.kv_heads, self.scale)

    def _hidden_residual_norm(self, tokens, pos, slot, tiles, n_dec, layers=None):
        """residual_in_gemm=False (A/B only): F.linear o / down projections and
        residual-add RMSNorm kernels instead of beta = 1 GEMM epilogues."""
        cfg, ops = self.cfg, self.ops
        layers = self.layers if layers is None else layers
        h = F.embedding(tokens, self.embed)
        res = h.clone()
        x = ops.rmsnorm(h, layers[0]["attn_norm"], cfg.eps)
        out = None
        for i, L in enumerate(layers):
            if i > 0:
                x = ops.rmsnorm(out, L["attn_norm"], cfg.eps, residual=res)
            a = self._attend(self._qkv(x, L, i, pos, slot), i, pos, slot, tiles, n_dec)
            x2 = ops.rmsnorm(F.linear(a, L["wo"]), L["mlp_norm"], cfg.eps, residual=res)
            act = ops.mlp_up(x2, L["w_gu"], self.fused_mlp, self.min_fused_tokens)
            out = F.linear(act, L["w_down"])
        return ops.rmsnorm(out, self.final_norm, cfg.eps, residual=res)
