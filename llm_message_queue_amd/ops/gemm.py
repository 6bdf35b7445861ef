"""Hand-written gfx950 GEMMs (``csrc/kernels/gemm_kernels.h``, ``skinny_kernels.h``).

The 256x256-tile kernel, one launch per call, by epilogue: ``gemm`` (plain
``x·Wᵀ``), ``gemm_swiglu`` (the Llama MLP's ``silu(x·Wgᵀ) * (x·Wuᵀ)`` over a
:func:`swiglu_permute`-d weight: inside every 256-column tile each wave's 64
columns are 32 gate features then the same 32 up features, so g and u of one
element share a lane and the gate/up product never reaches HBM), ``qkv_rope``
(qkv projection + RoPE + K/V-cache write), ``gemm_residual`` /
``gemm_residual_rms`` (``res += x·Wᵀ`` in place, the second with the next
RMSNorm's row scales) and ``lm_head_argmax`` / ``lm_head_sample`` (the LM head
with greedy or per-row temperature sampling, no logits tensor;
``sample_truncated`` is the top-k / top-p sampler over given logits,
``csrc/kernels/sample_truncate_kernels.h``, ``token_logprobs`` scores a
token and the most likely alternatives over given logits,
``csrc/kernels/logprob_kernels.h``).  The first
three take ``row_scale`` (the folded RMSNorm).  A step too small to fill the
CUs runs split-K (:func:`split_plan`, :func:`split_all`) or, below
``SKINNY_*_MAX_M`` rows, on the skinny kernel (:func:`skinny`; :func:`skinny_fp8`
over FP8 weight codes, :func:`quantize_rows` to make them -- ``ops.quant``).
``gemm_fp8`` / ``gemm_swiglu_fp8`` / ``gemm_residual_fp8`` are the tile kernel
over the same FP8 codes (``gemm_fp8w_kernel`` in ``gemm_kernels.h``); :func:`fp8_plan` says which
of the two FP8 kernels a quant forward's GEMM takes.

CPU / reference path: :func:`swiglu_reference` (fp32 math of the same op).
"""
from __future__ import annotations

import functools

import torch

from .. import _native

EPI_STORE = 0
EPI_SWIGLU = 2
EPI_RESID = 5       # A/B: residual tile read into registers in the epilogue
EPI_RESID_LDS = 6   # residual tile staged into LDS by DMA, added in place (default)
EPI_RESID_PRE = 7   # A/B: ... its first quarter fetched into spare LDS at kernel start
# which residual epilogue ``gemm_residual`` launches (bench.py --resid-epi)
RESID_EPI = EPI_RESID_LDS
TILE_M = 256
TILE_N = 256
SWIGLU_HALF = 32   # per-wave gate/up split (a wave owns 64 output columns)


def swiglu_perm_index(ffn: int, device=None, half: int = None) -> torch.Tensor:
    """Row order of the permuted [2F][K] weight: row r of the permuted
    matrix is row ``idx[r]`` of ``cat([W_gate, W_up])``.  Each wave's
    2*half output columns are ``half`` gate features then the same ``half``
    up features (the kernel: half = 32)."""
    half = half or SWIGLU_HALF
    if ffn % (TILE_N // 2):
        raise ValueError("ffn must be a multiple of 128")
    r = torch.arange(2 * ffn, device=device)
    tn, rem = r // TILE_N, r % TILE_N
    wc, rem2 = rem // (2 * half), rem % (2 * half)
    nh, c = rem2 // half, rem2 % half
    f = tn * (TILE_N // 2) + wc * half + c
    return torch.where(nh == 0, f, ffn + f)


def swiglu_permute(w_gu: torch.Tensor, half: int = None) -> torch.Tensor:
    """[gate; up] (2F x K) -> the fused kernel's row order (contiguous)."""
    ffn = w_gu.shape[0] // 2
    return w_gu.index_select(0, swiglu_perm_index(ffn, w_gu.device, half)).contiguous()


def swiglu_unpermute(w_perm: torch.Tensor, half: int = None) -> torch.Tensor:
    ffn = w_perm.shape[0] // 2
    idx = swiglu_perm_index(ffn, w_perm.device, half)
    out = torch.empty_like(w_perm)
    out.index_copy_(0, idx, w_perm)
    return out


def swiglu_reference(x: torch.Tensor, w_gu: torch.Tensor) -> torch.Tensor:
    """fp32 reference over the UNpermuted [gate; up] weight."""
    ffn = w_gu.shape[0] // 2
    gu = x.float() @ w_gu.float().t()
    return (torch.nn.functional.silu(gu[:, :ffn]) * gu[:, ffn:]).to(x.dtype)


def _check(t: torch.Tensor, name: str):
    if t.dtype != torch.bfloat16:
        raise TypeError(f"{name}: expected bfloat16, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if t.data_ptr() % 16:
        raise ValueError(f"{name} must be 16-byte aligned")


def supported(M: int, N: int, K: int) -> bool:
    return M > 0 and N % TILE_N == 0 and K % 128 == 0


def _tiles(M: int, N: int) -> int:
    return (M + TILE_M - 1) // TILE_M * (N // TILE_N)


def row_scale_len(M: int) -> int:
    """Floats a row_scale buffer must hold: the kernel reads whole 256-row
    tiles of it (rows past M are read but never stored)."""
    return (M + 255) // 256 * 256


def _row_scale_ptr(rs, M: int) -> int:
    if rs is None:
        return 0
    if rs.dtype != torch.float32 or not rs.is_contiguous() or rs.numel() < row_scale_len(M):
        raise ValueError("row_scale must be a contiguous float32 tensor of >= ceil(M/256)*256 values "
                         "(ops.llama_ops.HipOps.row_rms pads)")
    if rs.data_ptr() % 16:
        raise ValueError("row_scale must be 16-byte aligned")
    return rs.data_ptr()


_SCRATCH = {}   # (device type, device index, stream handle, user) -> (live tensors, retired tensors)


def _scratch_entry(device, stream: int, name: str):
    """The (live, retired) tensor lists of user ``name`` on one stream."""
    key = (device.type, device.index, stream, name)
    entry = _SCRATCH.get(key)
    if entry is None:
        entry = _SCRATCH[key] = ([], [])
    return entry


def _scratch(device, stream: int, name: str, *specs):
    """The kernels' grow-only scratch, one entry per (device, stream) and user
    ("split", "rms", "skinny", "head", "trunc", "pen"): the entry's tensors, one per
    ``(need, floor, alloc, dtype)`` in ``specs``.  A tensor of at least
    ``need`` elements is returned as it is, so launches in stream order share
    it and concurrent streams never do.  One too small is replaced by
    ``alloc`` (``torch.zeros`` for the counters the kernels find and leave
    zero, else ``torch.empty``) of ``max(need, floor, 2 * old)`` elements and
    moves to the entry's retired list, where it lives until
    :func:`drop_stream_scratch`: a captured graph or a launch in flight may
    still point at it, so the allocator must not hand it to anyone else.
    Growth at least doubles, which keeps the retired tensors together
    smaller than the live one."""
    live, retired = _SCRATCH.get((device.type, device.index, stream, name)) or _scratch_entry(device, stream, name)
    if not live:
        live.extend(alloc(max(need, floor), dtype=dtype, device=device) for need, floor, alloc, dtype in specs)
    for i, (need, floor, alloc, dtype) in enumerate(specs):
        old = live[i]
        if old.numel() < need:
            live[i] = alloc(max(need, floor, 2 * old.numel()), dtype=dtype, device=device)
            retired.append(old)
    return live


def drop_stream_scratch(stream: int) -> None:
    """Forget every scratch tensor, live and retired, of stream handle
    ``stream`` on any device (before the stream is destroyed: nothing that
    was allocated on it may be freed after, and a new stream reusing the
    handle must not inherit them)."""
    for key in [k for k in _SCRATCH if k[2] == stream]:
        del _SCRATCH[key]


def split_all(M: int, N: int, K: int, cus: int):
    """Split-K for a step too small to fill ``cus`` CUs with whole tiles:
    every tile runs as two K-half blocks (returns 0 = the first whole
    tile index) when twice the tiles still fit one wave, else None."""
    tiles = _tiles(M, N)
    if cus <= 0 or 2 * tiles > cus or K % 256 or K < 512:
        return None
    return 0


def _launch(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, epi: int, group_m: int = 8, row_scale=None,
            split_cus: int = 0):
    k = _native.require_hipops()
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError("gemm: inner dimensions differ")
    if not supported(M, N, K):
        raise ValueError(f"gemm: unsupported shape M={M} N={N} K={K}")
    stream = torch.cuda.current_stream(x.device).cuda_stream
    k.gemm_bf16(x.data_ptr(), w.data_ptr(), out.data_ptr(), M, N, K, epi, stream, group_m,
                _row_scale_ptr(row_scale, M), *_split_args(x.device, stream, M, N, K, split_cus))
    return out


def _split_args(device, stream: int, M: int, N: int, K: int, split_cus: int):
    """The launchers' ``(split_full, workspace, counters)`` for ``split_cus``
    CUs: every tile split (:func:`split_all`), else only a half-empty last
    wave (:func:`split_plan`), else (0, 0, 0) = whole tiles."""
    f = None
    if split_cus:
        f = split_all(M, N, K, split_cus)
        f = split_plan(M, N, K, split_cus) if f is None else f
    if f is None:
        return 0, 0, 0
    n_split = _tiles(M, N) - f
    w_t, c_t = _split_workspace(device, stream, n_split, max(split_cus, 2 * n_split))
    return f, w_t.data_ptr(), c_t.data_ptr()


def gemm(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor = None, row_scale=None,
         split_cus: int = 0) -> torch.Tensor:
    """x [M][K] · w[N][K]ᵀ -> [M][N] bf16 on the hand-written kernel
    (``row_scale`` [M] fp32: output row i is multiplied by row_scale[i];
    ``split_cus``: run split-K when the tiles cannot fill that many CUs,
    :func:`split_all`, or on a half-empty last wave, :func:`split_plan`)."""
    _check(x, "x")
    _check(w, "w")
    y = out if out is not None else torch.empty((x.shape[0], w.shape[0]), dtype=x.dtype, device=x.device)
    _check(y, "out")
    return _launch(x, w, y, EPI_STORE, row_scale=row_scale, split_cus=split_cus)


def gemm_swiglu(x: torch.Tensor, w_perm: torch.Tensor, out: torch.Tensor = None, row_scale=None,
                split_cus: int = 0) -> torch.Tensor:
    """silu(x·Wgᵀ) * (x·Wuᵀ) -> [M][F] bf16, ``w_perm`` from :func:`swiglu_permute`.
    ``row_scale`` [M] fp32 scales row i of both products first: with the
    RMSNorm weight folded into W and row_scale = ``row_rms(x)`` this is the
    MLP of rmsnorm(x) without materialising the normalised rows."""
    _check(x, "x")
    _check(w_perm, "w_perm")
    F = w_perm.shape[0] // 2
    y = out if out is not None else torch.empty((x.shape[0], F), dtype=x.dtype, device=x.device)
    _check(y, "out")
    if y.shape != (x.shape[0], F):
        raise ValueError("gemm_swiglu: out shape mismatch")
    return _launch(x, w_perm, y, EPI_SWIGLU, row_scale=row_scale, split_cus=split_cus)


def _rms_workspace(device, stream: int, tiles_m: int, tiles_n: int):
    """Scratch of the fused row-scale epilogue: fp32 row partials [tiles_m *
    tiles_n * 256] and int tickets [tiles_m] (zero; every launch leaves them zero)."""
    return _scratch(device, stream, "rms",
                    (tiles_m * tiles_n * 256, tiles_m * max(tiles_n, 16) * 256, torch.empty, torch.float32),
                    (tiles_m, 0, torch.zeros, torch.int32))


def gemm_residual_rms(x: torch.Tensor, w: torch.Tensor, res: torch.Tensor, eps: float) -> torch.Tensor:
    """``res += x · wᵀ`` (the LDS-DMA residual epilogue) and, in the same
    launch, the RMSNorm row scale of the updated ``res``: returns fp32
    [row_scale_len(M)] holding ``1 / sqrt(mean(res[r]^2) + eps)`` for rows
    r < M -- ``HipOps.row_rms(res, eps)`` without its separate pass over the
    rows (the next fused GEMM applies it per row).  Sums of squares are
    added in a fixed order, so the result is deterministic; it matches
    ``row_rms`` to fp32 rounding of a different summation order."""
    _check(x, "x")
    _check(w, "w")
    _check(res, "res")
    M, K = x.shape
    N = w.shape[0]
    if w.dim() != 2 or w.shape[1] != K:
        raise ValueError("gemm_residual_rms: inner dimensions differ")
    if not supported(M, N, K):
        raise ValueError(f"gemm_residual_rms: unsupported shape M={M} N={N} K={K}")
    if res.shape != (M, N):
        raise ValueError("gemm_residual_rms: res shape mismatch")
    if w.device != x.device or res.device != x.device:
        raise ValueError("gemm_residual_rms: w / res must be on x's device")
    stream = torch.cuda.current_stream(x.device).cuda_stream
    tiles_m, tiles_n = (M + TILE_M - 1) // TILE_M, N // TILE_N
    part, ticket = _rms_workspace(x.device, stream, tiles_m, tiles_n)
    scale = torch.empty(row_scale_len(M), dtype=torch.float32, device=x.device)
    _native.require_hipops().gemm_residual_rms(x.data_ptr(), w.data_ptr(), res.data_ptr(), M, N, K, stream,
                                               8, part.data_ptr(), ticket.data_ptr(), scale.data_ptr(),
                                               float(eps))
    return scale


def gemm_residual(x: torch.Tensor, w: torch.Tensor, res: torch.Tensor, split_cus: int = 0) -> torch.Tensor:
    """``res += x · wᵀ`` in place (bf16 ``res`` [M][N]; the fp32 sum is
    rounded once, as hipBLASLt's beta = 1 epilogue) -- the o / down
    projections accumulating into the residual stream.  Pulling the residual
    tile into L2 during the K-loop drain (4 or 8 MFMA phases ahead of the
    epilogue) was measured at +0.0-0.1 % (no gain: the epilogue is not
    waiting on the read; profiles/r3_gemm_resid_prefetch_ab.jsonl), so the
    plain epilogue stays."""
    _check(x, "x")
    _check(w, "w")
    _check(res, "res")
    if res.shape != (x.shape[0], w.shape[0]):
        raise ValueError("gemm_residual: res shape mismatch")
    if split_cus and RESID_EPI != EPI_RESID_LDS:
        split_cus = 0                                  # (split-K is wired for the LDS epilogue only)
    return _launch(x, w, res, RESID_EPI, split_cus=split_cus)


def residual_tiles_ok(M: int, N: int, cus: int, min_fill: float = 0.97) -> bool:
    """Whether the 256x256-tile kernel fills the chip for ``res += x·wᵀ``:
    the last wave of tiles at least ``min_fill`` busy.  On a partial wave
    (e.g. 128 tiles on 256 CUs) hipBLASLt's stream-K kernel splits K across
    the idle CUs and stays ahead (profiles/r2_gemm_resid_ab.jsonl)."""
    if not supported(M, N, 128) or N % TILE_N:
        return False
    tiles = _tiles(M, N)
    waves = -(-tiles // cus)
    return tiles / (waves * cus) >= min_fill


def split_plan(M: int, N: int, K: int, cus: int):
    """Split-K for the last, partial wave of tiles: returns ``full`` (tiles
    run whole) or None.  The kernel holds one block per CU, so ``tiles`` over
    ``cus`` CUs is ceil(tiles / cus) waves; when the last wave is at most half
    full its tiles run as two blocks over one K-half each (one wave of
    ``cus`` becomes half a wave).  qkv at the serving shape: 16 x 24 = 384
    tiles on 256 CUs -> 256 whole + 128 split."""
    tiles = _tiles(M, N)
    tail = tiles % cus
    if tiles <= cus or tail == 0 or 2 * tail > cus or K % 256 or K < 512:
        return None
    return tiles - tail


def _split_workspace(device, stream: int, n_split: int, cus: int):
    """fp32 slabs (256 KiB per split tile) + zeroed ticket/ready counters,
    sized for the largest possible tail (cus / 2).  The kernel re-zeroes the
    counters it used, so launches in stream order can share them."""
    cap = max(cus // 2, n_split)
    return _scratch(device, stream, "split", (n_split * 512 * 128, cap * 512 * 128, torch.empty, torch.float32),
                    (n_split * 2, cap * 2, torch.zeros, torch.int32))


@functools.lru_cache(maxsize=None)
def _cu_count_idx(index: int) -> int:
    return torch.cuda.get_device_properties(index).multi_processor_count


# device index -> CUs the serving steps' stream may use, when the chip is
# split into CU partitions (backend.cu_partition): wave / split-K plans are
# sized for the partition, not the whole chip
EFFECTIVE_CUS = {}


def _cu_count(device) -> int:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return EFFECTIVE_CUS.get(idx) or _cu_count_idx(idx)


def qkv_rope(x: torch.Tensor, wqkv: torch.Tensor, pos: torch.Tensor, slot: torch.Tensor,
             cos_t: torch.Tensor, sin_t: torch.Tensor, Hq: int, Hkv: int,
             kc: torch.Tensor, vc: torch.Tensor, q_out: torch.Tensor = None, row_scale=None,
             split: bool = True, split_full: int = None, group_m: int = 8) -> torch.Tensor:
    """The qkv projection with RoPE + the K/V cache write as its epilogue:
    returns q [T][Hq*128] (rotated) and writes this step's K/V rows into
    ``kc`` / ``vc`` [slots][Hkv][max_ctx][128] -- the same result as
    ``F.linear`` followed by ``HipOps.rope_kv``, without the [T][qkv]
    intermediate or the second launch.  ``row_scale`` as in :func:`gemm_swiglu`
    (applied to q, k and v before the rotation).  ``split``: run a partial
    last wave of tiles split-K (:func:`split_plan`)."""
    _check(x, "x")
    _check(wqkv, "wqkv")
    for t, n in ((kc, "kc"), (vc, "vc")):
        _check(t, n)
    if pos.dtype != torch.int32 or slot.dtype != torch.int32 or not (pos.is_contiguous() and slot.is_contiguous()):
        raise TypeError("pos / slot must be contiguous int32")
    if cos_t.dtype != torch.float32 or sin_t.dtype != torch.float32 or cos_t.shape[1] != 64:
        raise TypeError("cos / sin tables must be float32 [max_ctx][64]")
    T, K = x.shape
    S, hk, max_ctx, hd = kc.shape
    if hk != Hkv or hd != 128 or vc.shape != kc.shape or cos_t.shape[0] < max_ctx:
        raise ValueError("kv cache / rope table shape mismatch")
    if pos.numel() != T or slot.numel() != T:
        raise ValueError("pos / slot length must equal the token count")
    if wqkv.dim() != 2 or wqkv.shape[1] != K:
        raise ValueError("qkv_rope: inner dimensions differ")
    q = q_out if q_out is not None else torch.empty((T, Hq * 128), dtype=x.dtype, device=x.device)
    _check(q, "q_out")
    if tuple(q.shape) != (T, Hq * 128):
        raise ValueError(f"qkv_rope: q_out shape {tuple(q.shape)} != {(T, Hq * 128)}")
    for t, n in ((wqkv, "wqkv"), (pos, "pos"), (slot, "slot"), (cos_t, "cos_t"), (sin_t, "sin_t"), (kc, "kc"),
                 (vc, "vc"), (q, "q_out")):
        if t.device != x.device:
            raise ValueError(f"qkv_rope: {n} must be on x's device")
    k = _native.require_hipops()
    N = wqkv.shape[0]
    full, ws, cnt = 0, 0, 0
    stream = torch.cuda.current_stream(x.device).cuda_stream
    if split:
        cus = _cu_count(x.device)
        f = split_plan(T, N, K, cus) if split_full is None else split_full
        if f is not None:
            n_split = _tiles(T, N) - f
            w_t, c_t = _split_workspace(x.device, stream, n_split, cus)
            full, ws, cnt = f, w_t.data_ptr(), c_t.data_ptr()
    k.gemm_qkv_rope(x.data_ptr(), wqkv.data_ptr(), T, N, K, pos.data_ptr(), slot.data_ptr(),
                    cos_t.data_ptr(), sin_t.data_ptr(), Hq, Hkv, max_ctx, S, q.data_ptr(), kc.data_ptr(),
                    vc.data_ptr(), stream, _row_scale_ptr(row_scale, T), full, ws, cnt, group_m)
    return q


# ---------------------------------------------------------------------- skinny small steps
SKINNY_MAX_M = 64              # the model's gate/up on the skinny kernel up to this many rows
SKINNY_PROJ_MAX_M = 256        # ... and qkv up to this many (profiles/r6_skinny_chunked.jsonl)
SKINNY_RESID_MAX_M = 512       # ... and o / down (into the residual) up to this many (profiles/r6_skinny_mid_m.jsonl)
SKINNY_CHUNKED_MAX_M = 1024    # the kernel itself: 128-row chunks of A up to this many rows
SK_STORE, SK_RESID, SK_SWIGLU = 0, 1, 2


def skinny_splits(N: int, K: int, cus: int, M: int = 1) -> int:
    """Split-K factor of a skinny GEMM: the fewest K-splits that give at
    least two blocks (128 columns x one 128-row chunk of M) per CU, each
    split a multiple of 128 deep and at least 512."""
    blocks = N // 128 * max(1, -(-M // 128))
    best = 1
    for s in (1, 2, 4, 7, 8, 14, 16):
        if K % (128 * s) or K // s < 512:
            continue
        best = s
        if blocks * s >= 2 * cus:
            break
    return best


def _skinny_args(fn: str, x: torch.Tensor, wshape, out: torch.Tensor, epi: int, row_scale, cus: int, splits: int):
    """What :func:`skinny` and :func:`skinny_fp8` (``fn``, for the messages)
    share once their operands are checked: the shapes against the weight's
    ``wshape`` [N][K], the split-K factor, the scratch and the row scale.
    Returns the launch's ``(M, N, K, epi, row-scale pointer, scratch pointer,
    S, stream)``."""
    if out.device != x.device or (row_scale is not None and row_scale.device != x.device):
        raise ValueError(f"{fn}: out / row_scale must be on x's device")
    if x.device.type != "cuda":
        raise ValueError(f"{fn}: x must be on a GPU")
    M, K = x.shape
    N = wshape[0]
    if wshape[1] != K or not 1 <= M <= SKINNY_CHUNKED_MAX_M or N % 128 or K % 128:
        raise ValueError(f"{fn}: unsupported shape M={M} N={N} K={K}")
    want = (M, N // 2) if epi == SK_SWIGLU else (M, N)
    if tuple(out.shape) != want:
        raise ValueError(f"{fn}: out shape {tuple(out.shape)} != {want}")
    S = splits or skinny_splits(N, K, cus, M)
    if K % (128 * S):
        raise ValueError(f"{fn}: K={K} does not split {S} ways in 128-deep steps")
    stream = torch.cuda.current_stream(x.device).cuda_stream
    ws, = _scratch(x.device, stream, "skinny", (S * M * N, SKINNY_MAX_M * 32768, torch.empty, torch.float32))
    rs = 0
    if row_scale is not None:
        if row_scale.dtype != torch.float32 or not row_scale.is_contiguous() or row_scale.numel() < M:
            raise ValueError(f"{fn}: row_scale must be contiguous float32 [>= M]")
        rs = row_scale.data_ptr()
    return M, N, K, epi, rs, ws.data_ptr(), S, stream


def skinny(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, epi: int, row_scale=None, cus: int = 32,
           splits: int = 0):
    """``out`` (+)= ``x`` [M <= 1024][K] . ``w`` [N][K]^T on the skinny kernel
    (``csrc/kernels/skinny_kernels.h``): SK_STORE (out [M][N]), SK_RESID
    (out += ..., one rounding), SK_SWIGLU (``w`` swiglu-permuted, out [M][N/2]);
    ``row_scale`` multiplies row i of the product first (the folded RMSNorm).
    ``cus``: CUs the launch may use (the split-K factor is sized for them);
    ``splits`` > 0 forces the split-K factor (measurements)."""
    _check(x, "x")
    _check(w, "w")
    _check(out, "out")
    if w.device != x.device:
        raise ValueError("skinny: w must be on x's device")
    args = _skinny_args("skinny", x, w.shape, out, epi, row_scale, cus, splits)
    _native.require_hipops().skinny_gemm(x.data_ptr(), w.data_ptr(), out.data_ptr(), *args)
    return out


def skinny_fp8(x: torch.Tensor, codes: torch.Tensor, col_scale: torch.Tensor, out: torch.Tensor, epi: int,
               row_scale=None, cus: int = 32, splits: int = 0):
    """:func:`skinny` over FP8 weights (W8A16): ``codes`` uint8 [N][K] e4m3fn
    and ``col_scale`` float32 [N], one scale a weight row (``ops.quant``), so
    ``out (+)= (x . codesᵀ) * col_scale[n] * row_scale[m]`` -- the codes are
    decoded to bf16 in registers, the scales applied in fp32 by the finalize
    kernel.  Under SK_SWIGLU ``codes`` / ``col_scale`` follow the
    swiglu-permuted row order.  Same shapes, split-K rule, scratch and
    determinism as :func:`skinny`."""
    _check(x, "x")
    _check(out, "out")
    if codes.dtype != torch.uint8 or codes.dim() != 2 or not codes.is_contiguous() or codes.data_ptr() % 16:
        raise ValueError("skinny_fp8: codes must be contiguous 16-byte-aligned uint8 [N][K]")
    N = codes.shape[0]
    if col_scale.dtype != torch.float32 or tuple(col_scale.shape) != (N,) or not col_scale.is_contiguous() \
            or col_scale.data_ptr() % 16:
        raise ValueError("skinny_fp8: col_scale must be contiguous 16-byte-aligned float32 [N]")
    if codes.device != x.device or col_scale.device != x.device:
        raise ValueError("skinny_fp8: codes / col_scale must be on x's device")
    args = _skinny_args("skinny_fp8", x, codes.shape, out, epi, row_scale, cus, splits)
    _native.require_hipops().skinny_gemm_fp8(x.data_ptr(), codes.data_ptr(), col_scale.data_ptr(), out.data_ptr(),
                                             *args)
    return out


# ---------------------------------------------------------------------- FP8-weight 256x256 tiles
# Rows from which a quant forward's GEMM leaves the skinny kernel for the
# FP8-weight tile kernel (gemm_fp8w_kernel, csrc/kernels/gemm_kernels.h), by GEMM of the
# layer: on a micro-forward's CU partition (SMALL) and on the whole chip.
# Every value is >= 65: the graph buckets stop at 64 rows, so decode-sized
# micro-forwards and captured graphs keep the skinny kernel.  A value above
# SKINNY_CHUNKED_MAX_M means never.  Each is the smallest measured M from
# which the tile kernel beats skinny_fp8 by more than skinny_fp8's spread at
# every larger M (profiles/fp8_tile_gemm_ab.jsonl, rows of that GEMM and
# place; profiles/fp8_tile.md section 1): on 64 CUs qkv 0.96x at 128 and 1.51x at 192,
# o 0.97x at 256 and 1.46x at 384, gate/up 1.008x at 65 already (spread
# 0.4 %), down 0.66x at 128 and 1.11x at 192; on the chip the skinny kernel's
# chunks spread over 256 CUs and hold out longer: qkv 0.76x at 256 and 1.016x
# at 384, gate/up 0.96x at 65 and 1.09x at 96, o and down only at 1,024 rows
# (1.05x, 1.27x; 0.71x, 0.74x at 512).
FP8_GEMMS = ("qkv", "o", "gu", "down")
FP8_TILE_MIN_M_SMALL = {"qkv": 192, "o": 384, "gu": 65, "down": 192}
FP8_TILE_MIN_M_CHIP = {"qkv": 384, "o": 1024, "gu": 96, "down": 1024}


def fp8_plan(M: int, gemm: str, small: bool) -> str:
    """Which FP8 kernel GEMM ``gemm`` ("qkv", "o", "gu", "down") of a quant
    forward takes at ``M`` rows: "skinny" or "tile".  ``small``: on a
    micro-forward's CU partition.  Never "tile" at M <= SKINNY_MAX_M (the
    graph buckets) or above SKINNY_CHUNKED_MAX_M (no quant forward is that
    large)."""
    table = FP8_TILE_MIN_M_SMALL if small else FP8_TILE_MIN_M_CHIP
    if gemm not in table:
        raise ValueError(f"fp8_plan: unknown GEMM {gemm!r}")
    return "tile" if max(table[gemm], SKINNY_MAX_M + 1) <= M <= SKINNY_CHUNKED_MAX_M else "skinny"


def _launch_fp8(fn: str, x: torch.Tensor, codes: torch.Tensor, col_scale: torch.Tensor, out: torch.Tensor,
                epi: int, row_scale=None, split_cus: int = 0):
    """What the FP8-weight tile wrappers share: the checks of ``codes`` /
    ``col_scale`` (as :func:`skinny_fp8`), the shape, the split-K plan and its
    workspace (as :func:`_launch`: the same "split" scratch entry)."""
    _check(x, "x")
    _check(out, "out")
    if codes.dtype != torch.uint8:
        raise TypeError(f"{fn}: codes must be uint8, got {codes.dtype}")
    if codes.dim() != 2 or not codes.is_contiguous() or codes.data_ptr() % 16:
        raise ValueError(f"{fn}: codes must be contiguous 16-byte-aligned uint8 [N][K]")
    N = codes.shape[0]
    if col_scale.dtype != torch.float32 or tuple(col_scale.shape) != (N,) or not col_scale.is_contiguous() \
            or col_scale.data_ptr() % 16:
        raise ValueError(f"{fn}: col_scale must be contiguous 16-byte-aligned float32 [N]")
    if codes.device != x.device or col_scale.device != x.device or out.device != x.device:
        raise ValueError(f"{fn}: codes / col_scale / out must be on x's device")
    if x.dim() != 2 or codes.shape[1] != x.shape[1]:
        raise ValueError(f"{fn}: inner dimensions differ")
    M, K = x.shape
    if not supported(M, N, K):
        raise ValueError(f"{fn}: unsupported shape M={M} N={N} K={K}")
    want = (M, N // 2) if epi == EPI_SWIGLU else (M, N)
    if tuple(out.shape) != want:
        raise ValueError(f"{fn}: out shape {tuple(out.shape)} != {want}")
    rs = _row_scale_ptr(row_scale, M)
    k = _native.require_hipops()
    stream = torch.cuda.current_stream(x.device).cuda_stream
    k.gemm_fp8w(x.data_ptr(), codes.data_ptr(), col_scale.data_ptr(), out.data_ptr(), M, N, K, epi, stream, 8,
                rs, *_split_args(x.device, stream, M, N, K, split_cus))
    return out


def gemm_fp8(x: torch.Tensor, codes: torch.Tensor, col_scale: torch.Tensor, out: torch.Tensor = None,
             row_scale=None, split_cus: int = 0) -> torch.Tensor:
    """:func:`gemm` over FP8 weights (W8A16, ``ops.quant``): ``codes`` uint8
    [N][K] e4m3fn and ``col_scale`` float32 [N], the tensors of
    :func:`skinny_fp8`; ``out = (x . codesᵀ) * col_scale[n] * row_scale[m]``
    on the 256x256-tile kernel, the codes decoded to bf16 in registers.  With
    power-of-two scales bit-equal to :func:`gemm` over the decoded weights."""
    y = out if out is not None else torch.empty((x.shape[0], codes.shape[0]), dtype=x.dtype, device=x.device)
    return _launch_fp8("gemm_fp8", x, codes, col_scale, y, EPI_STORE, row_scale, split_cus)


def gemm_swiglu_fp8(x: torch.Tensor, codes_perm: torch.Tensor, col_scale_perm: torch.Tensor,
                    out: torch.Tensor = None, row_scale=None, split_cus: int = 0) -> torch.Tensor:
    """:func:`gemm_swiglu` over FP8 weights: ``codes_perm`` / ``col_scale_perm``
    follow the :func:`swiglu_permute`-d row order (the gate and the up row of
    a feature carry their own scales) -> [M][F] bf16."""
    y = out if out is not None else torch.empty((x.shape[0], codes_perm.shape[0] // 2), dtype=x.dtype,
                                                device=x.device)
    return _launch_fp8("gemm_swiglu_fp8", x, codes_perm, col_scale_perm, y, EPI_SWIGLU, row_scale, split_cus)


def gemm_residual_fp8(x: torch.Tensor, codes: torch.Tensor, col_scale: torch.Tensor, res: torch.Tensor,
                      split_cus: int = 0) -> torch.Tensor:
    """:func:`gemm_residual` over FP8 weights: ``res += (x . codesᵀ) *
    col_scale[n]`` in place, one rounding of the fp32 sum (the LDS-DMA
    residual epilogue).  Takes no row scale, as :func:`gemm_residual`."""
    return _launch_fp8("gemm_residual_fp8", x, codes, col_scale, res, EPI_RESID_LDS, None, split_cus)


def quantize_rows(w: torch.Tensor):
    """(codes uint8 [N][K], scale float32 [N]) of the bf16 rows ``w`` on the
    device kernel -- bit for bit ``ops.quant.quantize_rows_e4m3``."""
    _check(w, "w")
    if w.dim() != 2 or w.shape[1] % 8 or not w.shape[1]:
        raise ValueError("quantize_rows: w must be [N][K], K a positive multiple of 8")
    if not bool(torch.isfinite(w).all()):
        raise ValueError("quantize_rows: non-finite weight")
    N, K = w.shape
    codes = torch.empty((N, K), dtype=torch.uint8, device=w.device)
    scale = torch.empty(N, dtype=torch.float32, device=w.device)
    _native.require_hipops().quant_rows_e4m3(w.data_ptr(), N, K, codes.data_ptr(), scale.data_ptr(),
                                             torch.cuda.current_stream(w.device).cuda_stream)
    return codes, scale


def fp8_decode(codes: torch.Tensor) -> torch.Tensor:
    """The device decode of e4m3 ``codes`` (uint8, 1-D, a multiple of 4
    long): int16 bf16 bit patterns, one a code."""
    if codes.dtype != torch.uint8 or codes.dim() != 1 or codes.numel() % 4 or not codes.is_contiguous():
        raise ValueError("fp8_decode: codes must be contiguous uint8 [4 n]")
    out = torch.empty(codes.numel(), dtype=torch.int16, device=codes.device)
    _native.require_hipops().fp8_decode(codes.data_ptr(), codes.numel(), out.data_ptr(),
                                        torch.cuda.current_stream(codes.device).cuda_stream)
    return out


def _head_scratch(device, stream: int, M: int, N: int):
    """[M][N/256] (value, column) partials of the LM-head epilogues."""
    n = M * (N // TILE_N)
    return _scratch(device, stream, "head", (n, 0, torch.empty, torch.float32), (n, 0, torch.empty, torch.int32))


def _head_args(fn: str, x: torch.Tensor, w: torch.Tensor, out):   # checks, scratch, the int32 [M] output
    _check(x, "x")
    _check(w, "w")
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K or not supported(M, N, K):
        raise ValueError(f"{fn}: unsupported shape M={M} N={N} K={K}")
    y = out if out is not None else torch.empty(M, dtype=torch.int32, device=x.device)
    if y.dtype != torch.int32 or y.numel() < M or not y.is_contiguous():
        raise ValueError(f"{fn}: out must be contiguous int32 [M]")
    stream = torch.cuda.current_stream(x.device).cuda_stream
    return M, N, K, stream, _head_scratch(x.device, stream, M, N), y


def lm_head_argmax(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """Greedy next tokens ``argmax_n (x . w[n])`` -> int32 [M] with the argmax
    in the GEMM epilogue: no [M][vocab] logits tensor is written or re-read
    (the LM head of the serving step: ~1k rows x 128k vocab).  Ties resolve
    to the lower index as torch.argmax does; the values compared are the fp32
    accumulators, not bf16-rounded logits.  Scratch [M][N/256] (value, column)
    partials are cached per (device, stream)."""
    M, N, K, stream, ws, y = _head_args("lm_head_argmax", x, w, out)
    _native.require_hipops().gemm_argmax(x.data_ptr(), w.data_ptr(), M, N, K, ws[0].data_ptr(), ws[1].data_ptr(),
                                         y.data_ptr(), stream)
    return y


def lm_head_sample(x: torch.Tensor, w: torch.Tensor, inv_temp: torch.Tensor, keys: torch.Tensor,
                   out: torch.Tensor = None) -> torch.Tensor:
    """Per-row temperature sampling ``argmax_n (x . w[n] * inv_temp + G(key,
    n))`` -> int32 [M] in the GEMM epilogue (``lm_head_argmax`` with the
    Gumbel noise of ``ops.sampling`` / ``sample_noise.h`` added to the scaled
    accumulators): an exact draw from ``softmax(logits / T)`` with no logits
    tensor and no softmax pass.  ``inv_temp`` float32 [>= M] (0: the row is
    greedy and equals ``lm_head_argmax``'s), ``keys`` 32-bit [>= M][2] =
    ``ops.sampling.row_keys``.  The kernel reads whole 256-row tiles of both:
    pass them ``row_scale_len(M)`` rows long (rows past M zero) or they are
    padded here.  Shares ``lm_head_argmax``'s scratch."""
    M, N, K, stream, ws, y = _head_args("lm_head_sample", x, w, out)
    if inv_temp.dtype != torch.float32 or inv_temp.dim() != 1 or inv_temp.numel() < M or inv_temp.device != x.device:
        raise ValueError("lm_head_sample: inv_temp must be float32 [>= M] on x's device")
    if keys.dtype not in (torch.int32, torch.uint32) or keys.dim() != 2 or keys.shape[1] != 2 \
            or keys.shape[0] < M or keys.device != x.device:
        raise ValueError("lm_head_sample: keys must be 32-bit [>= M][2] on x's device")
    Mp = row_scale_len(M)
    if inv_temp.numel() < Mp or not inv_temp.is_contiguous() or inv_temp.data_ptr() % 16:
        inv_temp = torch.nn.functional.pad(inv_temp[:M], (0, Mp - M))
    if keys.shape[0] < Mp or not keys.is_contiguous() or keys.data_ptr() % 16:
        keys = torch.nn.functional.pad(keys[:M].view(torch.int32), (0, 0, 0, Mp - M))
    _native.require_hipops().gemm_sample(x.data_ptr(), w.data_ptr(), M, N, K, inv_temp.data_ptr(), keys.data_ptr(),
                                         Mp, ws[0].data_ptr(), ws[1].data_ptr(), y.data_ptr(), stream)
    return y


def sample_truncated(logits: torch.Tensor, inv_temp: torch.Tensor, keys: torch.Tensor, top_k: torch.Tensor,
                     top_p: torch.Tensor, vocab: int = None, out: torch.Tensor = None,
                     log_min_p: torch.Tensor = None) -> torch.Tensor:
    """Top-k / top-p / min-p sampling over given bf16 ``logits`` [R][ld] -> int32 [R]
    (``csrc/kernels/sample_truncate_kernels.h`` holds the contract,
    ``ops.sampling.sample_truncated_reference`` is its twin): per row, top-k
    then top-p select whole groups of equal values, and the pick is the argmax
    of ``logit * inv_temp + G(key, n)`` over the kept columns.  ``vocab``:
    the columns that count (default ld; the rest of a row is padding), ``ld %
    8 == 0``.  ``inv_temp`` float32 [>= R] (> 0), ``keys`` 32-bit [>= R][2] =
    ``ops.sampling.row_keys``, ``top_k`` int32 [>= R] (0: off), ``top_p``
    float32 [>= R] (>= 1: off), ``log_min_p`` float32 [>= R] or None:
    ``ops.sampling.min_p_log`` of the row's ``min_p`` (-inf, or None: off)."""
    _check(logits, "logits")
    if logits.dim() != 2:
        raise ValueError("sample_truncated: logits must be [R][ld]")
    R, ld = logits.shape
    V = ld if vocab is None else int(vocab)
    if not 0 < V <= ld or ld % 8:
        raise ValueError(f"sample_truncated: needs 0 < vocab <= ld and ld % 8 == 0 (vocab={V} ld={ld})")
    for t, n, dt in ((inv_temp, "inv_temp", (torch.float32,)), (top_k, "top_k", (torch.int32,)),
                     (top_p, "top_p", (torch.float32,)), (log_min_p, "log_min_p", (torch.float32,))):
        if t is None:
            continue
        if t.dtype not in dt or t.dim() != 1 or t.numel() < R or not t.is_contiguous() or t.device != logits.device:
            raise ValueError(f"sample_truncated: {n} must be contiguous {dt[0]} [>= R] on the logits' device")
    if keys.dtype not in (torch.int32, torch.uint32) or keys.dim() != 2 or keys.shape[1] != 2 \
            or keys.shape[0] < R or not keys.is_contiguous() or keys.device != logits.device:
        raise ValueError("sample_truncated: keys must be contiguous 32-bit [>= R][2] on the logits' device")
    y = out if out is not None else torch.empty(R, dtype=torch.int32, device=logits.device)
    if y.dtype != torch.int32 or y.numel() < R or not y.is_contiguous() or y.device != logits.device:
        raise ValueError("sample_truncated: out must be contiguous int32 [>= R] on the logits' device")
    _native.require_hipops().sample_truncated(logits.data_ptr(), R, V, ld, inv_temp.data_ptr(), keys.data_ptr(),
                                              top_k.data_ptr(), top_p.data_ptr(), y.data_ptr(),
                                              torch.cuda.current_stream(logits.device).cuda_stream,
                                              log_min_p.data_ptr() if log_min_p is not None else 0)
    return y[:R]


from .sampling import LP_TOP  # noqa: E402  (alternatives a row)


def token_logprobs(logits: torch.Tensor, tok: torch.Tensor, vocab: int = None, out_lp: torch.Tensor = None,
                   out_id: torch.Tensor = None):
    """Log-probabilities over given bf16 ``logits`` [R][ld] -> ``(lp float32
    [R][1 + LP_TOP], ids int32 [R][LP_TOP])`` (``csrc/kernels/
    logprob_kernels.h`` holds the contract, ``ops.sampling.logprob_reference``
    is its twin): per row ``log_softmax`` over the finite columns, of token
    ``tok[r]`` first (-inf for a token out of range or on a non-finite column),
    then of the LP_TOP most likely columns ``ids`` (ties to the lower column;
    -1 / -inf where the row has fewer).  ``vocab``: the columns that count
    (default ld; the rest of a row is padding), ``ld % 8 == 0``.  ``tok`` int32
    [>= R]."""
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or not logits.is_cuda:
        raise ValueError("token_logprobs: logits must be bfloat16 [R][ld] on a GPU")
    R, ld = logits.shape
    if R:                                               # (an empty tensor has no address to check)
        _check(logits, "logits")
    V = ld if vocab is None else int(vocab)
    if not 0 < V <= ld or ld % 8:
        raise ValueError(f"token_logprobs: needs 0 < vocab <= ld and ld % 8 == 0 (vocab={V} ld={ld})")
    if tok.dtype != torch.int32 or tok.dim() != 1 or tok.numel() < R or not tok.is_contiguous() \
            or tok.device != logits.device:
        raise ValueError("token_logprobs: tok must be contiguous int32 [>= R] on the logits' device")
    lp = out_lp if out_lp is not None else torch.empty((R, 1 + LP_TOP), dtype=torch.float32, device=logits.device)
    ids = out_id if out_id is not None else torch.empty((R, LP_TOP), dtype=torch.int32, device=logits.device)
    if lp.dtype != torch.float32 or lp.numel() < R * (1 + LP_TOP) or not lp.is_contiguous() \
            or lp.device != logits.device:
        raise ValueError("token_logprobs: out_lp must be contiguous float32 [>= R][6] on the logits' device")
    if ids.dtype != torch.int32 or ids.numel() < R * LP_TOP or not ids.is_contiguous() or ids.device != logits.device:
        raise ValueError("token_logprobs: out_id must be contiguous int32 [>= R][5] on the logits' device")
    if R:
        _native.require_hipops().logprobs(logits.data_ptr(), R, V, ld, tok.data_ptr(), lp.data_ptr(), ids.data_ptr(),
                                          torch.cuda.current_stream(logits.device).cuda_stream)
    return lp.view(-1)[:R * (1 + LP_TOP)].view(R, 1 + LP_TOP), ids.view(-1)[:R * LP_TOP].view(R, LP_TOP)


from .sampling import PEN_HIST_MAX  # noqa: E402  (history entries a row)


def _pen_logits(fn: str, logits: torch.Tensor, vocab):
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or not logits.is_cuda or not logits.is_contiguous():
        raise ValueError(f"{fn}: logits must be contiguous bfloat16 [R][ld] on a GPU")
    R, ld = logits.shape
    if R:
        _check(logits, "logits")
    V = ld if vocab is None else int(vocab)
    if not 0 < V <= ld or ld % 8:
        raise ValueError(f"{fn}: needs 0 < vocab <= ld and ld % 8 == 0 (vocab={V} ld={ld})")
    return R, ld, V


def _pen_hist(fn: str, hist: torch.Tensor, device):
    if hist.dtype != torch.int32 or hist.dim() != 2 or not hist.is_contiguous() or hist.device != device \
            or hist.numel() == 0 or hist.numel() >= 1 << 31:
        raise ValueError(f"{fn}: hist must be contiguous int32 [slots][stride] on the same device")


def penalise(logits: torch.Tensor, hist: torch.Tensor, spans: torch.Tensor, params: torch.Tensor,
             vocab: int = None) -> torch.Tensor:
    """Edit bf16 ``logits`` [R][ld] in place by the presence / frequency /
    repetition penalties of their rows' token histories (``csrc/kernels/
    penalty_kernels.h`` holds the contract, ``ops.sampling.
    penalise_rows_reference`` is its bit-exact twin).  ``hist`` int32
    [slots][stride <= PEN_HIST_MAX], ``spans`` int32 [>= R][4] = (slot, from,
    split, end): row r's history is ``hist[slot][from:end]``, its first
    ``split - from`` entries prompt tokens; ``params`` float32 [>= R][3] =
    (presence, frequency, repetition).  ``vocab``: the columns that count
    (default ld).  Returns ``logits``."""
    R, ld, V = _pen_logits("penalise", logits, vocab)
    _pen_hist("penalise", hist, logits.device)
    if hist.shape[1] > PEN_HIST_MAX:
        raise ValueError(f"penalise: a history of {hist.shape[1]} entries exceeds PEN_HIST_MAX = {PEN_HIST_MAX}")
    for t, n, dt, w in ((spans, "spans", torch.int32, 4), (params, "params", torch.float32, 3)):
        if t.dtype != dt or t.dim() != 2 or t.shape[1] != w or t.shape[0] < R or not t.is_contiguous() \
                or t.device != logits.device:
            raise ValueError(f"penalise: {n} must be contiguous {dt} [>= R][{w}] on the logits' device")
    if R:
        _native.require_hipops().penalise(logits.data_ptr(), R, V, ld, hist.data_ptr(), hist.shape[0], hist.shape[1],
                                          spans.data_ptr(), params.data_ptr(),
                                          torch.cuda.current_stream(logits.device).cuda_stream)
    return logits


def penalised_argmax(logits: torch.Tensor, vocab: int = None, inv_temp: torch.Tensor = None,
                     out: torch.Tensor = None) -> torch.Tensor:
    """The greedy pick over (edited) bf16 ``logits`` [R][ld] -> int32 [R]:
    argmax over the finite columns < ``vocab``, ties to the lower column, 0
    for a row with none (``penalty_kernels.h``; twin ``ops.sampling.
    penalised_pick_reference``).  With ``inv_temp`` (float32 [>= R]) only the
    rows with ``inv_temp <= 0`` are written; the others keep ``out``'s value."""
    R, ld, V = _pen_logits("penalised_argmax", logits, vocab)
    if inv_temp is not None and (inv_temp.dtype != torch.float32 or inv_temp.dim() != 1 or inv_temp.numel() < R
                                 or not inv_temp.is_contiguous() or inv_temp.device != logits.device):
        raise ValueError("penalised_argmax: inv_temp must be contiguous float32 [>= R] on the logits' device")
    y = out if out is not None else torch.zeros(R, dtype=torch.int32, device=logits.device)
    if y.dtype != torch.int32 or y.dim() != 1 or y.numel() < R or not y.is_contiguous() or y.device != logits.device:
        raise ValueError("penalised_argmax: out must be contiguous int32 [>= R] on the logits' device")
    if R:
        _native.require_hipops().penalised_argmax(logits.data_ptr(), R, V, ld,
                                                  inv_temp.data_ptr() if inv_temp is not None else 0, y.data_ptr(),
                                                  torch.cuda.current_stream(logits.device).cuda_stream)
    return y[:R]


def history_record(hist: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor, slot: torch.Tensor,
                   rows: torch.Tensor) -> None:
    """``hist[slot[t]][pos[t]] = tok[t]`` for the token rows ``t`` in ``rows``
    (int32 [Q]) of a forward's ``tok`` (int64 [T]), ``pos`` and ``slot``
    (int32 [T]): the device-side token history the penalties read
    (``penalty_kernels.h``).  A row, slot or position out of range writes
    nothing."""
    if not hist.is_cuda:
        raise ValueError("history_record: hist must be on a GPU")
    _pen_hist("history_record", hist, hist.device)
    T = tok.numel()
    for t, n, dt, ln in ((tok, "tok", torch.int64, T), (pos, "pos", torch.int32, T), (slot, "slot", torch.int32, T),
                         (rows, "rows", torch.int32, rows.numel())):
        if t.dtype != dt or t.dim() != 1 or t.numel() != ln or not t.is_contiguous() or t.device != hist.device:
            raise ValueError(f"history_record: {n} must be contiguous {dt}, tok / pos / slot of one length, "
                             "on hist's device")
    Q = rows.numel()
    if Q and T:
        _native.require_hipops().history_record(hist.data_ptr(), hist.shape[0], hist.shape[1], tok.data_ptr(),
                                                pos.data_ptr(), slot.data_ptr(), T, rows.data_ptr(), Q,
                                                torch.cuda.current_stream(hist.device).cuda_stream)


from .sampling import LE_MAX  # noqa: E402  (entries a list)


def logit_edit(logits: torch.Tensor, ids: torch.Tensor, vals: torch.Tensor, spans: torch.Tensor,
               vocab: int = None) -> torch.Tensor:
    """Edit bf16 ``logits`` [R][ld] in place by their rows' allow lists and
    additive biases (``csrc/kernels/logit_edit_kernels.h`` holds the contract,
    ``ops.sampling.logit_edit_reference`` is its bit-exact twin).  ``ids``
    int32 [N] and ``vals`` float32 [N] are the flat lists, ``spans`` int32
    [>= R][4] = (allow_off, n_allow, bias_off, n_bias): row r's allow list is
    ``ids[allow_off:allow_off + n_allow]``, its bias entries ``(ids[bias_off +
    i], vals[bias_off + i])``; a count is capped at LE_MAX and a span clamped
    to the lists.  ``vocab``: the columns that count (default ld).  Returns
    ``logits``."""
    R, ld, V = _pen_logits("logit_edit", logits, vocab)
    if logits.data_ptr() % 16:
        raise ValueError("logit_edit: logits must be 16-byte aligned")
    for t, n, dt in ((ids, "ids", torch.int32), (vals, "vals", torch.float32)):
        if t.dtype != dt or t.dim() != 1 or not t.is_contiguous() or t.device != logits.device:
            raise ValueError(f"logit_edit: {n} must be contiguous {dt} [N] on the logits' device")
    if ids.numel() != vals.numel():
        raise ValueError("logit_edit: ids and vals must have one length")
    if spans.dtype != torch.int32 or spans.dim() != 2 or spans.shape[1] != 4 or spans.shape[0] < R \
            or not spans.is_contiguous() or spans.device != logits.device:
        raise ValueError("logit_edit: spans must be contiguous int32 [>= R][4] on the logits' device")
    if R and ids.numel():
        _native.require_hipops().logit_edit(logits.data_ptr(), R, V, ld, ids.data_ptr(), vals.data_ptr(),
                                            ids.numel(), spans.data_ptr(),
                                            torch.cuda.current_stream(logits.device).cuda_stream)
    return logits


from .sampling import STOP_ENT_WORDS, STOP_ROW_WORDS  # noqa: E402  (words a row record / an entry)


def stop_match(tok: torch.Tensor, hist, rows: torch.Tensor, ent: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """Per row the lowest stop entry that equals the tail of its generated
    tokens, the step's token ``tok[r]`` included, or -1 -> int32 [R]
    (``csrc/kernels/stop_kernels.h`` holds the contract, ``ops.sampling.
    stop_match_reference`` is its exact twin).  ``tok`` int32 [R]; ``hist``
    int32 [slots][stride], the device-side token history, or None where no
    row reads one; ``rows`` int32 [>= R][6] = (slot, gen_from, end,
    min_tokens, ent_off, n_ent); ``ent`` int32 [N][9] = (length, tokens oldest
    first)."""
    if tok.dtype != torch.int32 or tok.dim() != 1 or not tok.is_cuda or not tok.is_contiguous():
        raise ValueError("stop_match: tok must be contiguous int32 [R] on a GPU")
    R = tok.numel()
    if hist is not None:
        _pen_hist("stop_match", hist, tok.device)
    for t, n, w in ((rows, "rows", STOP_ROW_WORDS), (ent, "ent", STOP_ENT_WORDS)):
        if t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != w or not t.is_contiguous() or t.device != tok.device:
            raise ValueError(f"stop_match: {n} must be contiguous int32 [n][{w}] on tok's device")
    if rows.shape[0] < R:
        raise ValueError("stop_match: rows must hold a record for every row of tok")
    y = out if out is not None else torch.empty(R, dtype=torch.int32, device=tok.device)
    if y.dtype != torch.int32 or y.dim() != 1 or y.numel() < R or not y.is_contiguous() or y.device != tok.device:
        raise ValueError("stop_match: out must be contiguous int32 [>= R] on tok's device")
    if R:
        _native.require_hipops().stop_match(tok.data_ptr(), R, hist.data_ptr() if hist is not None else 0,
                                            hist.shape[0] if hist is not None else 0,
                                            hist.shape[1] if hist is not None else 0, rows.data_ptr(),
                                            ent.data_ptr() if ent.numel() else 0, ent.shape[0], y.data_ptr(),
                                            torch.cuda.current_stream(tok.device).cuda_stream)
    return y[:R]


def sample_bits(keys: torch.Tensor, n0: int, count: int) -> torch.Tensor:
    """The device noise generator's bits (int32 [n_keys][count], the uint32
    bit patterns) of columns ``n0 .. n0 + count`` under ``keys`` [n][2]."""
    if keys.dtype not in (torch.int32, torch.uint32) or keys.dim() != 2 or keys.shape[1] != 2 \
            or not keys.is_contiguous():
        raise ValueError("sample_bits: keys must be contiguous 32-bit [n][2]")
    out = torch.empty((keys.shape[0], count), dtype=torch.int32, device=keys.device)
    _native.require_hipops().sample_bits(keys.data_ptr(), keys.shape[0], int(n0) & 0xFFFFFFFF, int(count),
                                         out.data_ptr(), torch.cuda.current_stream(keys.device).cuda_stream)
    return out

