"""GPU tests (-m gpu) of engines with an FP8 KV cache and 8 query heads per kv head: decode goes through kernels/attention_fp8_mfma.hip, eagerly, in
captured graphs and launched ahead; block sizes the kernel does not take are refused at creation."""
import gc

import numpy as np
import pytest

import nvr_import
from test_engine_kv_fp8_gpu import ECFG, MODEL, PROMPTS

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu

MODEL8 = {**MODEL, "num_attention_heads": 8, "num_key_value_heads": 1, "head_dim": 64}


def test_fp8_gqa8_engine_graph_replay_equals_eager():
    nvr.check(nvr.lib().nvr_device_set(0))
    streams = []
    for eager in (1, 0):                                             # prefill + 6 greedy decode steps: per-step (tokens, logits)
        nvr.lib().nvr_seq_reset_id_counter()
        e = nvr.LLMEngine(nvr.Config(**{**ECFG, "kvcache_block_size": 64, "kv_cache_dtype": "fp8", "enforce_eager": eager}), nvr.ModelConfig(**MODEL8))
        for p in PROMPTS:
            e.add_request(p, nvr.SamplingParams(temperature=0.0, max_tokens=32, ignore_eos=True))
        stream = []
        for _ in range(7):
            rec = e.step()
            stream.append((rec["tokens"], e.model_runner.logits(rec["num_seqs"]).copy()))
        assert e.model_runner.kv_cache_dtype() == "fp8_e4m3" and not e.model_runner.last_decode_ragged()
        assert eager or e.ahead_launched() > 0                       # steps were launched ahead (async_decode at its default)
        streams.append(stream)
        del e
        gc.collect()
    for k, ((t1, l1), (t2, l2)) in enumerate(zip(*streams)):
        assert np.isfinite(l1).all()
        assert t1 == t2 and np.array_equal(l1, l2), f"step {k}: tokens or logit bits of the eager and the graph-replaying engine differ"


def test_fp8_gqa8_engine_refuses_blocks_below_the_64_key_step():
    with pytest.raises(nvr.NvrError) as ex:
        nvr.LLMEngine(nvr.Config(**{**ECFG, "kvcache_block_size": 16, "kv_cache_dtype": "fp8"}), nvr.ModelConfig(**MODEL8))
    assert ex.value.code == -10 and "block size" in str(ex.value), str(ex.value)
