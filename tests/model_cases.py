"""Cases for the tests of the Llama trunk's kernel wiring (``LlamaStub.hidden``
/ ``_mlp_block`` / ``forward``): the steps of a case, the weights it installs
into a model, a float64 twin of the trunk and the single wiring mutations the
cases must be able to see.

The twin, :func:`trunk_reference`, is written from the maths: embedding; per
layer RMSNorm, the qkv projection, rotate-half RoPE on the 64/64 split, its own
float64 K/V caches, causal grouped-query attention over ``pos + 1`` keys of the
row's slot, the o projection into the residual, RMSNorm, SwiGLU, the down
projection into the residual; the final norm.  It reads the model's stored
bf16 weights (``ops.quant.dequantize`` of the stored codes for a quant case)
and rounds nothing afterwards.  It shares no code with ``RefOps``, ``HipOps``
or ``ops.gemm`` except ``swiglu_unpermute``, which reads the stored ``w_gu``.

A *mutation* is one wiring error applied to the twin only -- never to a
kernel.  ``tests/test_model_cases_cpu.py`` checks that every mutation moves a
row of the twin by several times the rounding error of the ``RefOps`` trunk,
which is what lets ``tests/test_gpu_model_routes.py`` bound every route of the
HIP trunk by a small multiple of that error.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from llm_message_queue_amd.models.llama_stub import QUANT_NAMES, LlamaStub
from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops import quant as Qn
from llm_message_queue_amd.ops.llama_ops import make_tiles

F64 = torch.float64

# the single wiring errors of the twin (layer 1 unless said)
MUTATIONS = (
    "rope_pos",          # RoPE position + 1 on one row (its q and its k)
    "one_key_fewer",     # one row attends pos keys instead of pos + 1
    "gu_block_swap",     # one 32-feature block of gate and up exchanged
    "norm_unfolded_gu",  # the norm weight not folded into w_gu
    "down_k_tail",       # the last 128 of K dropped in the down projection
    "gu_scale_stale",    # gate/up row scale taken from the residual before the o projection
    "wrong_slot_cache",  # one row reads another slot's cache
    "kv_group",          # two q heads use the neighbouring kv group (layer 0)
    "final_norm_unit",   # the final norm weight left at 1
)

# step 1: (slot, tokens) prefilled from position 0, in row order.  The slot
# numbers are neither contiguous nor ascending; slot 1 is not touched again.
_STEP1 = ((9, 37), (1, 9), (6, 5), (3, 33))
_DECODE = (9, 3)                 # step 2's decode rows continue these slots
_CONTINUED = 6                   # step 2's first chunk continues this slot, across 32 and 64 keys
_CONTINUED_MAX = 70
_FRESH = (11, 0, 7, 4, 10, 2, 8, 5)
SLOTS = 12


@dataclass
class Step:
    tokens: torch.Tensor          # int64 [T]
    pos: torch.Tensor             # int32 [T]
    slot: torch.Tensor            # int32 [T]
    tiles: torch.Tensor           # int32 [n, 4] (make_tiles), the decode tiles first
    n_dec: int
    rows: torch.Tensor            # int64: the sampled rows

    def to(self, device):
        return Step(*(t.to(device) if torch.is_tensor(t) else t for t in
                      (self.tokens, self.pos, self.slot, self.tiles, self.n_dec, self.rows)))

    @property
    def args(self):
        return self.tokens, self.pos, self.slot


@dataclass
class Case:
    cfg: object
    layers: int
    seed: int
    q_gain: float
    max_ctx: int
    steps: List[Step]
    mut_row: int                  # the row of the last step the row mutations change
    mut_slot: int                 # the slot "wrong_slot_cache" reads instead
    slots: int = SLOTS
    _weights: dict = field(default_factory=dict)


def _segments(segs, n_dec, vocab, gen, rows):
    """A step from ``segs`` = [(slot, first position, tokens)] in row order."""
    start, pos, slot = [], [], []
    at = 0
    for sl, p0, n in segs:
        start.append(at)
        pos += list(range(p0, p0 + n))
        slot += [sl] * n
        at += n
    tiles = make_tiles(start, [s[2] for s in segs], [s[0] for s in segs], [s[1] for s in segs])
    assert all(int(tiles[i, 1]) == 1 for i in range(n_dec))
    return Step(torch.randint(0, vocab, (at,), generator=gen), torch.tensor(pos, dtype=torch.int32),
                torch.tensor(slot, dtype=torch.int32), torch.from_numpy(tiles).contiguous(), n_dec,
                torch.tensor(rows, dtype=torch.int64))


def spread_rows(T: int, m: int):
    """``m`` sampled rows of a ``T``-row step: the first (a decode row), the
    last and rows in between, most of them inside a chunk, not at its end."""
    if m >= T:
        return list(range(T))
    if m <= 0:
        return []
    if m == 1:
        return [T - 1]
    return sorted({round(i * (T - 1) / (m - 1)) for i in range(m)})


def make_case(cfg, T: int, layers: int = 2, seed: int = 0, q_gain: float = 2.0, m_rows: Optional[int] = None):
    """The two steps of a case whose second step has exactly ``T`` rows
    (``T`` >= 8): step 1 prefills four slots; step 2 is two decode rows, a
    chunk that continues a step-1 context across 32 and 64 keys, and fresh
    prefill chunks of uneven length.  ``m_rows``: how many rows step 2
    samples (default: about one in seven)."""
    if T < 8:
        raise ValueError("a case needs at least 8 rows in its second step")
    gen = torch.Generator().manual_seed(1000 + seed)
    seg1 = [(sl, 0, n) for sl, n in _STEP1]
    T1 = sum(n for _, n in _STEP1)
    step1 = _segments(seg1, 0, cfg.vocab, gen, spread_rows(T1, 9))
    have = dict(_STEP1)
    seg2 = [(sl, have[sl], 1) for sl in _DECODE]
    left = T - len(seg2)
    n = min(left, _CONTINUED_MAX)
    seg2.append((_CONTINUED, have[_CONTINUED], n))
    left -= n
    per = max(70, -(-left // len(_FRESH)))
    for sl in _FRESH:
        if left <= 0:
            break
        n = min(left, per)
        seg2.append((sl, 0, n))
        left -= n
    assert left == 0
    step2 = _segments(seg2, len(_DECODE), cfg.vocab, gen,
                      spread_rows(T, max(3, T // 7) if m_rows is None else m_rows))
    need = max(p0 + n for _, p0, n in seg1 + seg2)
    return Case(cfg, layers, seed, q_gain, max(128, -(-need // 64) * 64), [step1, step2],
                mut_row=len(_DECODE) + 2, mut_slot=_DECODE[0])


# ------------------------------------------------------------------------------------------ weights
def _raw_weights(case: Case, device):
    """The case's weights before any model layout: bf16, drawn once per
    device from the case's seed (std 0.02, the q rows of wqkv times
    ``q_gain``; the norm weights 1 + 0.3 N(0, 1))."""
    key = str(device)
    if key not in case._weights:
        cfg = case.cfg
        g = torch.Generator(device=device).manual_seed(7000 + case.seed)

        def w(*shape, std=0.02, mean=0.0):
            return (torch.randn(*shape, generator=g, device=device, dtype=torch.float32) * std + mean) \
                .to(torch.bfloat16)

        d, nq = cfg.dim, cfg.heads * cfg.head_dim
        out = {"embed": w(cfg.vocab, d), "lm_head": w(cfg.vocab, d), "final_norm": w(d, std=0.3, mean=1.0),
               "layers": []}
        for _ in range(case.layers):
            wqkv = w(nq + 2 * cfg.kv_heads * cfg.head_dim, d).float()
            wqkv[:nq] *= case.q_gain
            out["layers"].append({
                "attn_norm": w(d, std=0.3, mean=1.0), "wqkv": wqkv.to(torch.bfloat16), "wo": w(d, nq),
                "mlp_norm": w(d, std=0.3, mean=1.0), "w_gu": w(2 * cfg.ffn, d), "w_down": w(d, cfg.ffn)})
        case._weights[key] = out
    return case._weights[key]


def install(model: LlamaStub, case: Case, decoded_from: Optional[LlamaStub] = None):
    """Put the case's weights into ``model``, in the model's own layout: the
    norm weights folded with ``LlamaStub._fold_norm`` where the model folds
    (``fused_qkv`` / ``fused_mlp``) and left as norm weights where it does
    not, ``w_gu`` through ``_gu_layout``, the FP8 copy rebuilt with
    ``_quantize``.  Models of one case on one device get identical tensors.
    ``decoded_from`` (a ``small_weights="fp8"`` model of the same case): the
    four layer matrices are that model's decoded codes instead -- what the
    reference model of a quant route computes with."""
    if len(model.layers) != case.layers:
        raise ValueError("the model and the case differ in their layer count")
    raw = _raw_weights(case, model.device)
    model.embed, model.lm_head = raw["embed"].clone(), raw["lm_head"].clone()
    model.final_norm = raw["final_norm"].clone()
    model.case_norms = []
    for i, (L, R) in enumerate(zip(model.layers, raw["layers"])):
        model.case_norms.append((R["attn_norm"], R["mlp_norm"]))
        wqkv, an = R["wqkv"].clone(), R["attn_norm"].clone()
        w_gu, mn = R["w_gu"].clone(), R["mlp_norm"].clone()
        if model.fused_qkv:
            wqkv, an = model._fold_norm(wqkv, an)
        if model.fused_mlp:
            w_gu, mn = model._fold_norm(w_gu, mn)
        L.update(attn_norm=an, wqkv=wqkv, wo=R["wo"].clone(), mlp_norm=mn, w_gu=model._gu_layout(w_gu),
                 w_down=R["w_down"].clone())
        if model.small_weights == "fp8":
            L["fp8"] = {k: model._quantize(L[k]) for k in QUANT_NAMES}
        if decoded_from is not None:
            src = decoded_from.layers[i]["fp8"]
            if decoded_from.fused_mlp != model.fused_mlp:
                raise ValueError("decoded_from must keep w_gu in the model's layout")
            for k in QUANT_NAMES:
                L[k] = Qn.dequantize(*src[k])
    model.__dict__.pop("_deq_layers", None)
    for c in model.kcache + model.vcache:
        c.zero_()
    return model


# ------------------------------------------------------------------------------------------ the float64 twin
def _weights64(model: LlamaStub, quant: bool):
    out = []
    for L in model.layers:
        W = {}
        for k in QUANT_NAMES:
            W[k] = Qn.dequantize(*L["fp8"][k]) if quant else L[k]
        if model.fused_mlp:
            W["w_gu"] = G.swiglu_unpermute(W["w_gu"])
        W = {k: v.to(F64) for k, v in W.items()}
        W["attn_norm"], W["mlp_norm"] = L["attn_norm"].to(F64), L["mlp_norm"].to(F64)
        out.append(W)
    return out


def _norm_scale(x, eps):
    return torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)


def _rotate(v, ang):
    """Rotate-half RoPE: v [T, H, 128], ang [T, 64]."""
    c, s = ang.cos()[:, None, :], ang.sin()[:, None, :]
    a, b = v[..., :64], v[..., 64:]
    return torch.cat([a * c - b * s, b * c + a * s], dim=-1)


def _attention(q, kc, vc, src, nkeys, kvmap, scale, stats):
    """q [T, Hq, 128]; row t attends the first ``nkeys[t]`` positions of slot
    ``src[t]``; q head h reads kv head ``kvmap[h]``.  One pass per slot."""
    out = torch.empty_like(q)
    src_t = torch.tensor(src)
    n_t = torch.tensor(nkeys)
    for s in sorted(set(src)):
        idx = torch.nonzero(src_t == s).flatten()
        n = n_t[idx].to(q.device)
        idx = idx.to(q.device)
        nmax = int(n.max())
        K, V = kc[s, :, :nmax][kvmap], vc[s, :, :nmax][kvmap]           # [Hq, nmax, 128]
        sc = torch.einsum("thd,hnd->htn", q[idx], K) * scale
        keep = torch.arange(nmax, device=q.device)[None, :] < n[:, None]  # [t, nmax]
        if stats is not None:
            v = sc[:, keep]
            stats["n"] = stats.get("n", 0) + v.numel()
            stats["sum"] = stats.get("sum", 0.0) + float(v.sum())
            stats["sumsq"] = stats.get("sumsq", 0.0) + float((v * v).sum())
        p = torch.softmax(sc.masked_fill(~keep[None], -math.inf), dim=-1)
        out[idx] = torch.einsum("htn,hnd->thd", p, V)
    return out


def score_std(stats: dict) -> float:
    mean = stats["sum"] / stats["n"]
    return math.sqrt(max(stats["sumsq"] / stats["n"] - mean * mean, 0.0))


@torch.no_grad()
def trunk_reference(model: LlamaStub, steps, mutate: Optional[str] = None, quant: bool = False,
                    stats: Optional[dict] = None, mut_row: int = 0, mut_slot: int = 0):
    """Float64 hidden states [T, d] of every step of ``steps`` = [(tokens,
    pos, slot)], run in order on the twin's own caches, with ``model``'s
    weights.  ``mutate``: one of ``MUTATIONS``; the row mutations change row
    ``mut_row`` of the last step (``mut_slot``: the slot "wrong_slot_cache"
    reads).  ``stats`` collects the attention scores' moments
    (:func:`score_std`)."""
    if mutate is not None and mutate not in MUTATIONS:
        raise ValueError(f"unknown mutation {mutate!r}")
    cfg, dev = model.cfg, model.device
    Hq, Hkv, hd, eps = cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.eps
    W = _weights64(model, quant)
    embed, final = model.embed.to(F64), model.final_norm.to(F64)
    if mutate == "final_norm_unit":
        final = torch.ones_like(final)
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, 64, dtype=F64, device=dev) / 64.0))
    kc = [torch.zeros((model.slots, Hkv, model.max_ctx, hd), dtype=F64, device=dev) for _ in W]
    vc = [torch.zeros_like(k) for k in kc]
    scale = 1.0 / math.sqrt(hd)
    outs = []
    for si, (tokens, pos, slot) in enumerate(steps):
        hit = si == len(steps) - 1                       # the row mutations: the last step only
        pos_l, slot_l = [int(p) for p in pos.cpu()], [int(s) for s in slot.cpu()]
        T = len(pos_l)
        pos_d, slot_d = pos.to(dev).long(), slot.to(dev).long()
        x = embed[tokens.to(dev).long()]
        for i, L in enumerate(W):
            m = mutate if i == (0 if mutate == "kv_group" else 1) else None
            qkv = (x * _norm_scale(x, eps) * L["attn_norm"]) @ L["wqkv"].t()
            qkv = qkv.view(T, Hq + 2 * Hkv, hd)
            rpos = pos_d.clone()
            if m == "rope_pos" and hit:
                rpos[mut_row] += 1
            ang = rpos.to(F64)[:, None] * inv[None, :]
            q, k, v = _rotate(qkv[:, :Hq], ang), _rotate(qkv[:, Hq:Hq + Hkv], ang), qkv[:, Hq + Hkv:]
            kc[i][slot_d, :, pos_d] = k
            vc[i][slot_d, :, pos_d] = v
            src, nkeys = list(slot_l), [p + 1 for p in pos_l]
            kvmap = torch.arange(Hq, device=dev) // (Hq // Hkv)
            if m == "one_key_fewer" and hit:
                nkeys[mut_row] -= 1
            if m == "wrong_slot_cache" and hit:
                src[mut_row] = mut_slot
            if m == "kv_group":
                kvmap[:2] = (kvmap[:2] + 1) % Hkv
            a = _attention(q, kc[i], vc[i], src, nkeys, kvmap, scale, stats).reshape(T, Hq * hd)
            before = x
            x = x + a @ L["wo"].t()
            r = _norm_scale(before if m == "gu_scale_stale" else x, eps)
            w_gu, g = L["w_gu"], L["mlp_norm"]
            if m == "norm_unfolded_gu":
                g = torch.ones_like(g)
                if model.fused_mlp:                      # folded into the stored weight: take it out again
                    w_gu = w_gu / model.case_norms[i][1].to(F64)[None, :]
            gu = (x * r * g) @ w_gu.t()
            F = cfg.ffn
            gate, up = gu[:, :F], gu[:, F:]
            if m == "gu_block_swap":
                gate, up = gate.clone(), up.clone()
                gate[:, 32:64], up[:, 32:64] = gu[:, F + 32:F + 64], gu[:, 32:64]
            act = gate * torch.sigmoid(gate) * up
            if m == "down_k_tail":
                x = x + act[:, :F - 128] @ L["w_down"][:, :F - 128].t()
            else:
                x = x + act @ L["w_down"].t()
        outs.append(x * _norm_scale(x, eps) * final)
    return outs


def twin(model: LlamaStub, case: Case, mutate: Optional[str] = None, quant: bool = False, stats=None):
    """:func:`trunk_reference` over the case's steps and mutation rows."""
    return trunk_reference(model, [s.args for s in case.steps], mutate, quant=quant, stats=stats,
                           mut_row=case.mut_row, mut_slot=case.mut_slot)


# ------------------------------------------------------------------------------------------ the measure
def row_errors(h: torch.Tensor, h64: torch.Tensor) -> torch.Tensor:
    """Per row rms(h - h64) / rms(h64), float64."""
    h, h64 = h.to(F64), h64.to(h.device)
    return ((h - h64).pow(2).mean(-1) / h64.pow(2).mean(-1)).sqrt()


def run_steps(model: LlamaStub, case: Case, attention: str = "tiles", **kw):
    """``hidden`` of every step of the case on ``model`` (every row).
    ``attention``: "tiles" (the case's tiles and n_dec) or "tokens"."""
    outs = []
    for st in case.steps:
        st = st.to(model.device)
        if attention == "tiles":
            outs.append(model.hidden(*st.args, tiles=st.tiles, n_dec=st.n_dec, **kw))
        else:
            outs.append(model.hidden(*st.args, **kw))
    return outs
