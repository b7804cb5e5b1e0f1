"""GPU tests (-m gpu) of engines whose KV cache is FP8 (Config(kv_cache_dtype="fp8")).  Nothing here compares fp8-engine logits with 16-bit-engine
logits (quantisation error has no derivable bound; it is printed): the checks are the cache BYTES of layer 0 (which do not depend on the cache
dtype), eager == hipGraph replay, the pool size and the refusals."""
import gc

import numpy as np
import pytest

import nvr_import
from test_kv_fp8_gpu import e4m3_encode

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu

BS, VOCAB, NBLK = 16, 512, 32
MODEL = dict(vocab_size=VOCAB, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
             max_position_embeddings=2048, rope_theta=10000.0, tie_word_embeddings=False, init_std=0.05)
ECFG = dict(max_num_seqs=4, max_num_batched_tokens=256, max_model_len=256, kvcache_block_size=BS, num_kvcache_blocks=NBLK, skip_block_size_check=1,
            recompute_cached_prefix=1)
_base = nvr.synthetic_tokens(BS, 1, 0, VOCAB).tolist()               # two prompts share their first block
PROMPTS = [_base + nvr.synthetic_tokens(5, 1, 1, VOCAB).tolist(), _base + nvr.synthetic_tokens(9, 1, 2, VOCAB).tolist(), nvr.synthetic_tokens(11, 1, 3, VOCAB).tolist()]


def _run(scales=None, **cfg):
    """prefill + 6 greedy decode steps: per-step (tokens, logits), the sequences' (tokens, block table), layer 0's K and V cache as bytes"""
    nvr.check(nvr.lib().nvr_device_set(0))
    nvr.lib().nvr_seq_reset_id_counter()
    e = nvr.LLMEngine(nvr.Config(**{**ECFG, **cfg}), nvr.ModelConfig(**MODEL))
    if scales:
        e.model_runner.set_kv_scales(*scales)
    for p in PROMPTS:
        e.add_request(p, nvr.SamplingParams(temperature=0.0, max_tokens=32, ignore_eos=True))
    stream = []
    for _ in range(7):
        rec = e.step()
        stream.append((rec["tokens"], e.model_runner.logits(rec["num_seqs"]).copy()))
    seqs = [(s.token_ids, s.block_table) for s in e.last_batch()]
    nvr.synchronize()
    caches = [np.empty((NBLK * BS, 2 * 64 * (1 if scales else 2)), np.uint8) for _ in range(2)]
    for a, ptr in zip(caches, e.model_runner.kv_cache(0)):
        nvr.check(nvr.lib().nvr_memcpy_d2h(a.ctypes.data, ptr, a.nbytes))
    facts = (e.model_runner.kv_cache_dtype(), e.model_runner.last_shared_prefix_len(), e.model_runner.last_decode_ragged(), e.ahead_launched())
    if scales:
        with pytest.raises(nvr.NvrError) as ex:                      # the scales are fixed once a step has run
            e.model_runner.set_kv_scales(1.0, 1.0)
        assert ex.value.code == -6
    del e
    gc.collect()
    return stream, seqs, caches, facts


def test_fp8_engine_layer0_cache_bytes_are_the_encoded_16bit_rows():
    scales = (0.5, 2.0)
    fs, fseq, f8, ffacts = _run(scales=scales, kv_cache_dtype="fp8")
    ds, dseq, d16, dfacts = _run()
    assert ffacts[:3] == ("fp8_e4m3", 0, False) and dfacts[0] == "float16"
    fed = 1 + next((k for k, (a, b) in enumerate(zip(fs, ds)) if a[0] != b[0]), len(fs) - 1)    # steps whose input tokens were the same in both engines
    print(f"fp8 vs fp16 KV engine (an observation, no bound): max |dlogit| {max(np.abs(a[1] - b[1]).max() for a, b in zip(fs[:fed], ds[:fed])):.4f} over the {fed} steps "
          f"fed the same tokens (max |logit| {np.abs(ds[0][1]).max():.2f}); greedy tokens agree in {sum(a[0] == b[0] for a, b in zip(fs, ds))} / {len(fs)} steps")
    checked = 0
    for got8, want16, sc in zip(f8, d16, scales):
        want = want16.view(np.float16).astype(np.float64)
        for pr, (ftok, fbt), (dtok, dbt) in zip(PROMPTS, fseq, dseq):
            # position p was written by the step that fed token p (every position but the last); its layer-0 K / V rows follow from token and position
            # alone, so they are comparable wherever both engines fed the same token: the prompt and the first sampled token always are
            assert ftok[:len(pr)] == pr and dtok[:len(pr)] == pr
            same = [p for p in range(min(len(ftok), len(dtok)) - 1) if ftok[p] == dtok[p]]
            assert same[:len(pr) + 1] == list(range(len(pr) + 1))
            for p in same:
                frow, drow = fbt[p // BS] * BS + p % BS, dbt[p // BS] * BS + p % BS
                assert np.array_equal(got8[frow], e4m3_encode(want[drow] / sc)), f"layer-0 cache row of position {p} differs from the encoded 16-bit row"
                checked += 1
    assert checked >= 2 * (21 + 25 + 11 + 3)                         # K and V: every prompt position and the first decode-written slot of each sequence


def test_fp8_engine_graph_replay_equals_eager():
    eager = _run(kv_cache_dtype="fp8", enforce_eager=1)[0]
    graph, _, _, facts = _run(kv_cache_dtype="fp8", enforce_eager=0)
    assert facts[3] > 0                                              # steps were launched ahead (async_decode at its default)
    for k, ((t1, l1), (t2, l2)) in enumerate(zip(eager, graph)):
        assert t1 == t2 and np.array_equal(l1, l2), f"step {k}: tokens or logit bits of the eager and the graph-replaying engine differ"


def test_fp8_pool_size_and_refusals():
    nvr.check(nvr.lib().nvr_device_set(0))
    blocks = {}
    for kv in ("auto", "fp8"):                                       # one after the other: nearly the same free HBM
        r = nvr.ModelRunner(nvr.Config(**{**ECFG, "num_kvcache_blocks": "auto", "gpu_memory_utilization": 0.25, "kv_cache_dtype": kv}), nvr.ModelConfig(**MODEL))
        blocks[kv] = r.num_kvcache_blocks()
        del r
        gc.collect()
    assert blocks["fp8"] >= 1.9 * blocks["auto"], blocks
    for bad in (dict(recompute_cached_prefix=0), dict(enable_chunked_prefill=1), dict(dtype="float32")):
        with pytest.raises(nvr.NvrError) as ex:
            nvr.LLMEngine(nvr.Config(**{**ECFG, "kv_cache_dtype": "fp8", **bad}), nvr.ModelConfig(**MODEL))
        assert ex.value.code == -10 and ("dtype" in bad or ("recompute_cached_prefix" in str(ex.value) and "enable_chunked_prefill" in str(ex.value))), str(ex.value)
    with pytest.raises(nvr.NvrError) as ex:
        nvr.Config(kv_cache_dtype="int4").validate()
    assert ex.value.code == -7 and "Unsupported kv_cache_dtype: int4" in str(ex.value)
