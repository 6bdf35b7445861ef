"""The select of ``sample_truncated_kernel`` against rows whose kept set is
decided exactly (sampler_cases.py): cuts on the chunk, wave and window
boundaries of the histogram scan, tie arithmetic at the cut, every path of the
window loop, the +-0 group and subnormals, the whole key range, a high
inv_temp, and witnesses at the ends of the row and around the vector
boundaries.  Every row carries a searched key under which the twin's pick
wins clearly, so every assertion is equality with the twin: a kernel that
keeps one group too many picks the trap column, one that keeps one too few
loses the edge witness (test_sampler_cases_cpu.py shows both flips on the
host)."""
import time

import numpy as np
import pytest
import torch

import sampler_cases as SC
from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops import sampling as S

DEV = "cuda:0"
V_SERVE = 128256


def _upload(bits, V, it, keys, tk, tp, extra_ld=0):
    """bf16 bit patterns [R][V] -> the device arguments; the rows are ld =
    ceil(V / 8) * 8 + extra_ld long, the padding a huge finite logit that
    must never be counted or picked."""
    R = bits.shape[0]
    ld = (V + 7) // 8 * 8 + extra_ld
    d = torch.full((R, ld), 3.0e38, dtype=torch.bfloat16, device=DEV)
    d[:, :V] = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).to(DEV)
    return (d, torch.from_numpy(it).to(DEV), torch.from_numpy(np.ascontiguousarray(keys).view(np.int32)).to(DEV),
            torch.from_numpy(tk).to(DEV), torch.from_numpy(tp).to(DEV))


def _launch(bits, V, it, keys, tk, tp, extra_ld=0) -> list:
    got = G.sample_truncated(*_upload(bits, V, it, keys, tk, tp, extra_ld), vocab=V)
    assert got.dtype == torch.int32 and got.shape == (bits.shape[0],)
    return got.cpu().tolist()


def _report(V, tags, wants, got):
    kinds = [k for _c, k in tags]
    print(f"V={V}: {len({c.name for c, _k in tags})} cases, {len(wants)} rows: {kinds.count('edge')} edge witnesses, "
          f"{kinds.count('trap')} traps, {kinds.count('plain')} plain keys; witness search {SC.SEARCH_SECONDS[0]:.2f} s")
    for cls, (e, t, p) in sorted(SC.tally(tags).items()):
        print(f"  {cls}: {e} edge, {t} trap, {p} plain")
    for r, ((c, kind), w, g) in enumerate(zip(tags, wants, got)):
        if g != w:
            print(f"  row {r} {c.name} [{kind}] top_k={c.top_k} top_p={float(c.top_p):.6f}: got {g} "
                  f"(value {c.row64[g] if 0 <= g < V else None}, kept {bool(c.keep[g]) if 0 <= g < V else None}), twin {w}")


@pytest.mark.gpu
@pytest.mark.parametrize("V", [1003, 16384, 18437])
def test_every_case_picks_the_twins_column(V):
    """V = 1003: the masked loop of the row sweep only, threads without a
    column; 16,384: exactly one unmasked sweep, no tail; 18,437: an unmasked
    sweep and a masked tail, V % 8 = 5."""
    bits, it, keys, tk, tp, wants, tags = SC.witness_rows(SC.cases(V))
    SC.check_coverage(tags, V)
    t0 = time.perf_counter()
    got = _launch(bits, V, it, keys, tk, tp)
    print(f"launch and copies {time.perf_counter() - t0:.3f} s")
    _report(V, tags, wants, got)
    assert got == wants
    if V == 1003:
        # the row stride is not the vocabulary: 64 more columns of padding a row
        assert _launch(bits, V, it, keys, tk, tp, extra_ld=64) == wants


@pytest.mark.gpu
def test_window_edge_and_subnormal_cases_at_the_serving_vocabulary():
    bits, it, keys, tk, tp, wants, tags = SC.witness_rows(SC.cases(V_SERVE, SC.SERVING_CLASSES))
    SC.check_coverage(tags, V_SERVE, SC.SERVING_CLASSES)
    got = _launch(bits, V_SERVE, it, keys, tk, tp)
    _report(V_SERVE, tags, wants, got)
    assert got == wants


@pytest.mark.gpu
def test_a_row_sees_nothing_of_the_rows_its_block_did_before():
    """One launch of 528 rows on 256 blocks.  Rows 0..255 are dense (3 randn,
    top_k and top_p on, cuts in either window), so every block's histogram is
    full when it comes to its next row; rows 256..271 have no finite logit
    (the early exit, LDS untouched); rows 272..511 and 512..527 are the
    witness rows -- the last 16 directly after a row without a candidate on
    the same block.  Every witness row picks the twin's column, and the same
    column as in a launch of its own."""
    from llm_message_queue_amd import _native
    V, blocks, empty = 1003, _native.require_hipops().ST_MAX_BLOCKS, 16
    assert blocks == 256
    wb, wit, wkeys, wtk, wtp, wwants, tags = SC.witness_rows(SC.cases(V))
    n = blocks                                                        # witness rows: 240 after a dense row, 16 after an empty one
    pick = np.arange(n) % len(wwants)
    rng = np.random.default_rng(3)
    dense = S.bf16_bits((3.0 * rng.standard_normal((blocks, V))).astype(np.float32))
    bits = np.concatenate([dense, np.full((empty, V), 0x7FC0, dtype=np.uint16), wb[pick]])
    i = np.arange(blocks)
    it = np.concatenate([np.array([1.0, 0.5, 2.0], dtype=np.float32)[i % 3], np.ones(empty, dtype=np.float32), wit[pick]])
    tk = np.concatenate([np.array([900, 50, 1000, 5], dtype=np.int32)[i % 4], np.full(empty, 3, dtype=np.int32), wtk[pick]])
    tp = np.concatenate([np.array([0.9, 0.99999, 0.5], dtype=np.float32)[(i // 4) % 3], np.full(empty, 0.5, dtype=np.float32),
                         wtp[pick]])
    keys = np.concatenate([S.row_keys(np.arange(blocks + empty, dtype=np.uint64) + np.uint64(40), 0), wkeys[pick]])
    R = len(bits)
    assert R == 2 * blocks + empty and np.array_equal((np.arange(R)[-empty:]) % blocks, np.arange(empty))
    # the dense rows use both windows: top_k = 900 / 1000 of 1003 cuts among the negative values
    k0 = SC.st_key(dense)
    assert ((k0.max(axis=1)[:, None] - k0 >= SC.ST_WIN).sum(axis=1) > 300).all()
    args = _upload(bits, V, it, keys, tk, tp)
    got = G.sample_truncated(*args, vocab=V).cpu().tolist()
    want = [wwants[p] for p in pick]
    assert all(0 <= g < V for g in got[:blocks]) and got[blocks:blocks + empty] == [0] * empty
    _report(V, [tags[p] for p in pick], want, got[blocks + empty:])
    assert got[blocks + empty:] == want
    SC.check_coverage([tags[p] for p in pick[:len(wwants)]], V)
    alone = [int(G.sample_truncated(*(a[r:r + 1] for a in args), vocab=V).cpu()[0]) for r in range(blocks + empty, R)]
    assert alone == want
