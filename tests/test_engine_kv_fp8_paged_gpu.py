"""GPU tests (-m gpu) of FP8-KV engines whose prefill reads the byte cache through the block tables (kernels/flash_prefill_fp8.hip): a prompt's second
chunk and the same rows behind a cached prefix run the same arithmetic over the same bytes, and eager == hipGraph replay."""
import gc

import numpy as np

import nvr_import
import pytest
from test_engine_kv_fp8_gpu import MODEL, VOCAB

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu

ECFG = dict(max_num_seqs=4, max_num_batched_tokens=256, max_model_len=256, kvcache_block_size=64, num_kvcache_blocks=16, skip_block_size_check=1,
            kv_cache_dtype="fp8")
P = nvr.synthetic_tokens(104, 1, 7, VOCAB).tolist()
SP = dict(temperature=0.0, max_tokens=32, ignore_eos=True)


def _engine(**cfg):
    nvr.check(nvr.lib().nvr_device_set(0))
    nvr.lib().nvr_seq_reset_id_counter()
    return nvr.LLMEngine(nvr.Config(**{**ECFG, **cfg}), nvr.ModelConfig(**MODEL))


def _paged_step_then_decode(e, pid, decode_steps):
    """steps e until the prefill that feeds rows 64..103 of P (sequence pid) has run: that step's facts and P's logits, then P's next greedy tokens with their logits"""
    rec = e.step()
    seq = next(s for s in e.last_batch() if s.seq_id == pid)
    facts = (rec["is_prefill"], rec["num_seqs"], rec["num_tokens"], e.model_runner.last_prefill_kv_source())
    stream = [(rec["tokens"][rec["seq_ids"].index(pid)], e.model_runner.logits(rec["num_seqs"])[rec["seq_ids"].index(pid)].copy())]
    offsets = (seq.chunk, seq.num_cached_tokens)
    for _ in range(decode_steps):
        rec = e.step()
        i = rec["seq_ids"].index(pid)
        stream.append((rec["tokens"][i], e.model_runner.logits(rec["num_seqs"])[i].copy()))
    return facts, offsets, stream


def _cached_prefix_run(decode_steps, **cfg):
    """engine Y: P[:64] is prefilled whole (block 0), then P arrives and its prefill feeds rows 64..103 behind num_cached_tokens = 64"""
    e = _engine(recompute_cached_prefix=0, **cfg)
    e.add_request(P[:64], nvr.SamplingParams(**SP))
    first = e.step()
    assert first["is_prefill"] and first["num_tokens"] == 64 and e.model_runner.last_prefill_kv_source() == 0
    pid = e.add_request(P, nvr.SamplingParams(**SP))
    out = _paged_step_then_decode(e, pid, decode_steps)
    del e
    gc.collect()
    return out


def test_fp8_second_chunk_equals_the_rows_behind_a_cached_prefix():
    # (async_decode = 0: a step launched ahead would already have re-stamped the sequence's chunk fields when the prefill step returns)
    x = _engine(enable_chunked_prefill=1, max_num_batched_tokens=64, async_decode=0)
    pid = x.add_request(P, nvr.SamplingParams(**SP))
    first = x.step()                                                 # rows 0..63: a whole-prompt-style step over its own projections, writes block 0
    assert first["is_prefill"] and first["num_tokens"] == 64 and x.model_runner.last_prefill_kv_source() == 0
    xf, xo, xs = _paged_step_then_decode(x, pid, 4)
    del x
    gc.collect()
    yf, yo, ys = _cached_prefix_run(4, async_decode=0)
    # both are one prefill step of 40 tokens of one sequence that read K / V through the block tables, 64 tokens in
    assert xf == (True, 1, 40, 2) and yf == (True, 1, 40, 2), (xf, yf)
    assert xo[0] == (64, 40) and yo[1] == 64, (xo, yo)
    assert np.array_equal(xs[0][1], ys[0][1]), f"logits of the two routes differ by {np.abs(xs[0][1] - ys[0][1]).max()}"
    assert [t for t, _ in xs] == [t for t, _ in ys]


def test_fp8_paged_prefill_engine_graph_replay_equals_eager():
    ef, _, eager = _cached_prefix_run(6, enforce_eager=1)
    gf, _, graph = _cached_prefix_run(6, enforce_eager=0)
    assert ef == (True, 1, 40, 2) and gf == ef
    for k, ((t1, l1), (t2, l2)) in enumerate(zip(eager, graph)):
        assert t1 == t2 and np.array_equal(l1, l2), f"step {k}: tokens or logit bits of the eager and the graph-replaying engine differ"
