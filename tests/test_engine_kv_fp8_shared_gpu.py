"""GPU tests (-m gpu) of FP8-KV engines whose decode batches share a cached prefix: the step takes the shared-prefix attention pass over the byte cache
(nvr_paged_attn_decode_shared_fp8), eager and hipGraph replay agree bit for bit, and the pass changes the logits only within the attention tolerance."""
import gc

import numpy as np
import pytest

import nvr_import

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu

VOCAB, LOGIT_TOL = 512, 2e-2                                             # (LOGIT_TOL: tests/test_engine_gpu.py)
MODEL = dict(vocab_size=VOCAB, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
             max_position_embeddings=2048, rope_theta=10000.0, tie_word_embeddings=False, init_std=0.05)
ECFG = dict(max_num_seqs=8, max_num_batched_tokens=2048, max_model_len=512, kvcache_block_size=64, num_kvcache_blocks=48, skip_block_size_check=1,
            recompute_cached_prefix=1, kv_cache_dtype="fp8", shared_prefix_min_seqs=4)
_base = nvr.synthetic_tokens(150, 2, 0, VOCAB).tolist()                  # six prompts share two full blocks; the seventh is unrelated
PROMPTS = [_base + nvr.synthetic_tokens(n, 2, 1 + i, VOCAB).tolist() for i, n in enumerate((3, 9, 17, 26, 33, 40))]
PROMPTS.insert(3, nvr.synthetic_tokens(70, 2, 9, VOCAB).tolist())


@pytest.fixture(scope="module")
def runs():
    def run(**cfg):
        """prefill + 8 greedy decode steps: per step (tokens, logits, (num_seqs, shared length, shared rows))"""
        nvr.check(nvr.lib().nvr_device_set(0))
        nvr.lib().nvr_seq_reset_id_counter()
        e = nvr.LLMEngine(nvr.Config(**{**ECFG, **cfg}), nvr.ModelConfig(**MODEL))
        e.model_runner.set_kv_scales(0.5, 2.0)
        for p in PROMPTS:
            e.add_request(p, nvr.SamplingParams(temperature=0.0, max_tokens=32, ignore_eos=True))
        out = []
        for _ in range(9):
            rec = e.step()
            r = e.model_runner
            out.append((rec["tokens"], r.logits(rec["num_seqs"]).copy(), (rec["num_seqs"], r.last_shared_prefix_len(), r.last_shared_prefix_rows())))
        nvr.synchronize()
        del e
        gc.collect()
        return out
    return {"eager": run(enforce_eager=1), "graph": run(enforce_eager=0), "plain": run(enforce_eager=1, shared_prefix_min_seqs=-1)}


def test_fp8_engine_takes_the_shared_prefix_pass(runs):
    assert (7, 128, 6) in [s[2] for s in runs["eager"]] and (7, 128, 6) in [s[2] for s in runs["graph"]]
    assert all(s[2][1:] == (0, 0) for s in runs["plain"])


def test_fp8_engine_shared_prefix_graph_replay_equals_eager(runs):
    for k, ((t1, l1, _), (t2, l2, _)) in enumerate(zip(runs["eager"], runs["graph"])):
        assert t1 == t2 and np.array_equal(l1, l2), f"step {k}: tokens or logit bits of the eager and the graph-replaying engine differ"


def test_fp8_engine_shared_prefix_first_decode_step_logits(runs):
    """the first decode step reads the same cache bytes and inputs on both routes; measured max |dlogit| (MI355X): see DESIGN 6c"""
    k = next(i for i, s in enumerate(runs["eager"]) if s[2][1] > 0)
    (t1, l1, f1), (t2, l2, f2) = runs["eager"][k], runs["plain"][k]
    assert k >= 1 and runs["eager"][k - 1][2][1] == 0 and runs["eager"][k - 1][0] == runs["plain"][k - 1][0]   # the step in front is the (identical) prefill
    d = np.abs(l1 - l2).max()
    print(f"shared-prefix pass vs plain fp8 decode, first decode step: max |dlogit| {d:.3e} (max |logit| {np.abs(l2).max():.2f})")
    assert d < LOGIT_TOL
